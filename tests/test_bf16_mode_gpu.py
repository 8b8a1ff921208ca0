"""The opt-in bf16 convolution mode above the kernels: Learner.use_bf16_conv() on a resnet18 learner (which modules it marks, three
training steps eager and replayed from a captured graph, and back to the fp32 bits), and a BasicBlock in eval mode against an fp64
restatement of its forward on operands rounded as the kernels round them."""
import pytest
import torch
import torch.nn.functional as F

from test_dwconv_gpu import U, bounded
from tools.gen_golden_senet import WD, as_learner_model

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib
from neuralnetworklibrary_amd.Applications.VisionModels import resnet
from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import BasicBlock, HipConv2d
from neuralnetworklibrary_amd.General.Core import separate_bn_layers
from neuralnetworklibrary_amd.General.Learner import Learner

pytestmark = pytest.mark.gpu
DEV = 'cuda'


class Data:
    sz, categories, bs, target_type = (64, 64), {i: 'c%d' % i for i in range(5)}, 4, 'single_label'
    train_dl = val_dl = [(None, torch.zeros(4))]


def _steps(tmp_path, prepare):
    "(the learner, the losses of three steps, the parameters after them) of a freshly seeded resnet18 learner that `prepare` has set up"
    torch.manual_seed(0)
    net = as_learner_model(resnet.resnet18(num_classes=5), separate_bn_layers).to(DEV).train()
    learner = Learner(str(tmp_path), Data(), net, optimizer='SGD_Mom')
    learner.init_optimizer(wd=WD)
    assert prepare(learner) is learner
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(4, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 5, (4,), generator=g).to(DEV)
    losses = [learner.train1minibatch(x, y, [1e-2]) for _ in range(3)]
    return learner, losses, [p.detach().clone() for p in net.parameters()]


def test_use_bf16_conv_marks_trains_replays_and_restores(tmp_path):
    verbose, Learner.verbose = Learner.verbose, False
    try:
        runs = {name: _steps(tmp_path, prep) for name, prep in {
            'fp32': lambda l: l, 'bf16': lambda l: l.use_bf16_conv(), 'replayed': lambda l: l.use_graphs(warmup=1).use_bf16_conv(),
            'restored': lambda l: l.use_bf16_conv().use_bf16_conv(False)}.items()}
    finally:
        Learner.verbose = verbose
    convs = [m for m in runs['bf16'][0].model.modules() if isinstance(m, HipConv2d)]
    inside = [bool(lib.nnl_conv2d_bf16_supported(ops._geom(1, 9, 9, m.in_channels, m.out_channels, *m.kernel_size, m.stride[0], m.padding[0]))) for m in convs]
    assert [m.compute for m in convs] == ['bf16' if ok else 'fp32' for ok in inside] and sum(inside) == 19       # 16 block convs, 3 projections
    assert runs['bf16'][0].model.conv1.compute == 'fp32', 'the 3-channel stem is outside the domain'
    assert all(m.compute == 'fp32' for m in runs['restored'][0].model.modules() if isinstance(m, HipConv2d))
    print({k: v[1] for k, v in runs.items()})
    same = lambda a, b: runs[a][1] == runs[b][1] and all(torch.equal(p, q) for p, q in zip(runs[a][2], runs[b][2]))              # noqa: E731
    assert same('bf16', 'replayed'), 'the replayed steps differ from the eager ones'
    assert same('fp32', 'restored'), 'use_bf16_conv(False) does not restore the fp32 path'
    assert runs['bf16'][1] != runs['fp32'][1], 'the bf16 steps are the fp32 ones: the mode reached no kernel'


def test_basic_block_eval_forward_takes_the_bf16_route():
    g = torch.Generator().manual_seed(5)
    C, rb = 16, lambda t: t.bfloat16().double()
    block = BasicBlock(C, C)
    for bn in (block.bn1, block.bn2):
        bn.weight.data, bn.bias.data = 0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g)
        bn.running_mean.data, bn.running_var.data = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    x = torch.randn(2, C, 7, 9, generator=g).abs() + 1.0              # a positive shortcut: the closing ReLU clips next to nothing
    block = block.to(DEV).eval()
    with torch.no_grad():
        y32 = block(x.to(DEV))
        block.conv1.compute = block.conv2.compute = 'bf16'
        y16 = block(x.to(DEV))
    # the fp64 restatement, with the sums of absolute terms next to it; e1: what the fp32 y1 may be off by before it is rounded
    w1, w2 = rb(block.conv1.weight.detach().cpu()), rb(block.conv2.weight.detach().cpu())
    affine = lambda bn: ((bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().cpu().double().view(1, C, 1, 1),             # noqa: E731
                         bn.running_mean.detach().cpu().double().view(1, C, 1, 1), bn.bias.detach().cpu().double().view(1, C, 1, 1))
    (s1, m1, b1), (s2, m2, b2) = affine(block.bn1), affine(block.bn2)
    n = 9 * C + 3
    c1, a1 = F.conv2d(rb(x), w1, padding=1), F.conv2d(rb(x), w1.abs(), padding=1)
    y1 = torch.relu((c1 - m1) * s1 + b1)
    e1 = s1.abs() * (n * U * a1 + 8 * U * (a1 + m1.abs())) + 8 * U * b1.abs()
    c2, a2 = F.conv2d(rb(y1.float()), w2, padding=1), F.conv2d(y1, w2.abs(), padding=1)
    ref = torch.relu((c2 - m2) * s2 + b2 + x.double())
    # the kernel rounds an fp32 y1 that may round to the neighbouring bf16 of the fp64 one: one bf16 ulp, at most 2^-7 |y1| (or e1 next to zero)
    allowed = s2.abs() * ((2.0 ** -7 + n * U) * a2 + F.conv2d(e1, w2.abs(), padding=1)) + 8 * U * (s2.abs() * (a2 + m2.abs()) + b2.abs() + x.double())
    bounded('block forward', y16, ref, allowed / U, 1)
    differ = (y16 != y32).float().mean().item()
    print('bf16 output differs from the fp32 path on %.3f of the elements' % differ)
    assert differ > 0.5, 'the block did not reach the bf16 kernels'
