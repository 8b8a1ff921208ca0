"""The opt-in bf16 convolution mode on a grouped model: Learner.use_bf16_conv() on a one-block-per-stage SE-ResNeXt learner (Cg = Kg = 4, 8, 16,
32 from stage to stage) at 64 x 64 — which HipGroupedConv2d modules it marks, three training steps eager and replayed from a captured graph,
back to the fp32 bits, and that the switch on the grouped modules alone reaches the kernels of csrc/gconv_bf16.hip."""
import pytest
import torch

from tools.gen_golden_senet import WD, as_learner_model

from neuralnetworklibrary_amd._lib import lib
from neuralnetworklibrary_amd.Applications.VisionModels import senet
from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipGroupedConv2d
from neuralnetworklibrary_amd.General.Core import separate_bn_layers
from neuralnetworklibrary_amd.General.Learner import Learner

pytestmark = pytest.mark.gpu
DEV = 'cuda'


class Data:
    sz, categories, bs, target_type = (64, 64), {i: 'c%d' % i for i in range(5)}, 4, 'single_label'
    train_dl = val_dl = [(None, torch.zeros(4))]


def _grouped(learner):
    return [m for m in learner.model.modules() if isinstance(m, HipGroupedConv2d)]


def _only_grouped(learner):
    for m in _grouped(learner):
        m.compute = 'bf16'
    return learner


def _steps(tmp_path, prepare):
    "(the learner, the losses of three steps, the parameters after them) of a freshly seeded learner that `prepare` has set up"
    torch.manual_seed(0)
    net = senet.SENet(senet.SEResNeXtBottleneck, [1, 1, 1, 1], groups=32, reduction=16, dropout_p=None, inplanes=64, input_3x3=False,
                      downsample_kernel_size=1, downsample_padding=0, num_classes=5)
    net.avg_pool = torch.nn.AdaptiveAvgPool2d(1)                      # (a 64 x 64 input leaves 2 x 2 after layer4: the fixed AvgPool2d(7) refuses it)
    net = as_learner_model(net, separate_bn_layers).to(DEV).train()
    learner = Learner(str(tmp_path), Data(), net, optimizer='SGD_Mom')
    learner.init_optimizer(wd=WD)
    assert prepare(learner) is learner
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(4, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 5, (4,), generator=g).to(DEV)
    losses = [learner.train1minibatch(x, y, [1e-2]) for _ in range(3)]
    return learner, losses, [p.detach().clone() for p in net.parameters()]


def test_use_bf16_conv_marks_grouped_trains_replays_and_restores(tmp_path):
    verbose, Learner.verbose = Learner.verbose, False
    try:
        runs = {name: _steps(tmp_path, prep) for name, prep in {
            'fp32': lambda l: l, 'bf16': lambda l: l.use_bf16_conv(), 'replayed': lambda l: l.use_graphs(warmup=1).use_bf16_conv(),
            'restored': lambda l: l.use_bf16_conv().use_bf16_conv(False), 'grouped': _only_grouped}.items()}
    finally:
        Learner.verbose = verbose
    convs = _grouped(runs['bf16'][0])
    inside = [bool(lib.nnl_gconv2d_bf16_supported(1, 9, 9, m.in_channels, m.out_channels, m.groups, m.kernel_size[0], m.stride[0], m.padding[0]))
              for m in convs]
    assert [m.compute for m in convs] == ['bf16' if ok else 'fp32' for ok in inside] and sum(inside) == len(convs) == 4
    assert all(m.compute == 'fp32' for m in _grouped(runs['restored'][0]))
    print({k: v[1] for k, v in runs.items()})
    same = lambda a, b: runs[a][1] == runs[b][1] and all(torch.equal(p, q) for p, q in zip(runs[a][2], runs[b][2]))              # noqa: E731
    assert same('bf16', 'replayed'), 'the replayed steps differ from the eager ones'
    assert same('fp32', 'restored'), 'use_bf16_conv(False) does not restore the fp32 path'
    assert runs['grouped'][1] != runs['fp32'][1], 'the steps with the grouped modules on bf16 are the fp32 ones: the switch reached no kernel'
