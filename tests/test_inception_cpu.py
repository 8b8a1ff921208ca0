"""InceptionV4 without a GPU: state_dict keys / shapes and parameter order against golden G28 (tools/gen_golden_inception.py: the real
reference under torch.device('meta')), the domain checks of HipLineConv2d and ops.line_conv2d (raised before any device is needed), and
the host logic of the registry."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import inceptionv4, vmods
from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipConv2d, HipLineConv2d


def test_state_dict_keys_and_shapes_are_the_reference():
    with open(os.path.join(GOLDEN, 'g28_inception_keys.json')) as f:
        want = json.load(f)['inceptionv4']
    with torch.device('meta'):
        net = vmods.inceptionv4()
    assert isinstance(net, vmods.InceptionV4) and net.last_linear.out_features == 1000 and net.input_size == (299, 299, 3)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want
    buffers = ('running_mean', 'running_var', 'num_batches_tracked')
    assert [n for n, _ in net.named_parameters()] == [k for k, _ in want if not k.endswith(buffers)]
    convs = [m.conv for m in net.modules() if isinstance(m, inceptionv4.BasicConv2d)]
    assert len(convs) == 149 and sum(isinstance(c, HipLineConv2d) for c in convs) == 64
    assert all(isinstance(c, HipConv2d) == (c.kernel_size[0] == c.kernel_size[1]) for c in convs)
    assert all(m.bn.eps == 0.001 for m in net.modules() if isinstance(m, inceptionv4.BasicConv2d))


def test_domain_checks_name_the_argument_before_any_device():
    x = torch.zeros(1, 8, 9, 9)
    for match, call in [
            ('kernel_size', lambda: ops.line_conv2d(x, torch.zeros(8, 8, 3, 3))),
            ('kernel_size', lambda: ops.line_conv2d(x, torch.zeros(8, 8, 1, 4))),
            ('kernel_size', lambda: ops.line_conv2d(x, torch.zeros(8, 8, 9, 1))),
            ('kernel_size', lambda: ops.line_conv2d(x, torch.zeros(8, 8, 1, 1))),
            ('in_channels', lambda: ops.line_conv2d(torch.zeros(1, 6, 9, 9), torch.zeros(8, 6, 1, 3))),
            ('in_channels', lambda: ops.line_conv2d(x, torch.zeros(8, 4, 1, 3))),
            ('out_channels', lambda: ops.line_conv2d(x, torch.zeros(6, 8, 3, 1))),
            ('4-D', lambda: ops.line_conv2d(x[0], torch.zeros(8, 8, 1, 3))),
            ('kernel_size', lambda: HipLineConv2d(8, 8, 3, padding=1)(x)),
            ('kernel_size', lambda: HipLineConv2d(8, 8, (1, 9), padding=(0, 4))(x)),
            ('padding', lambda: HipLineConv2d(8, 8, (1, 7), padding=(3, 0))(x)),
            ('padding', lambda: HipLineConv2d(8, 8, (7, 1), padding=(3, 3))(x)),
            ('padding', lambda: HipLineConv2d(8, 8, (1, 3), padding=(0, 1), padding_mode='reflect')(x)),
            ('stride', lambda: HipLineConv2d(8, 8, (1, 3), stride=2, padding=(0, 1))(x)),
            ('dilation', lambda: HipLineConv2d(8, 8, (1, 3), padding=(0, 1), dilation=2)(x)),
            ('groups', lambda: HipLineConv2d(8, 8, (1, 3), padding=(0, 1), groups=2)(x))]:
        with pytest.raises(NotImplementedError, match=match):
            call()
    conv = HipLineConv2d(8, 12, (7, 1), padding=(3, 0), bias=False)
    assert not hasattr(conv, 'nnl_hip_conv') and conv.weight.permute(0, 2, 3, 1).is_contiguous()
    assert list(conv.state_dict()) == ['weight'] and conv.weight.shape == (12, 8, 7, 1)


def test_registry_factory_cut_split_and_feature_count():
    for pretrained in ('imagenet', 'imagenet+background'):
        with pytest.raises(RuntimeError, match='never downloads'):
            vmods.inceptionv4(pretrained=pretrained)
    with torch.device('meta'):
        net = vmods.inceptionv4(num_classes=7)
    assert net.last_linear.out_features == 7
    body = V.default_cut(net)
    assert body is net.features and len(list(body.children())) == 22
    assert [len(list(g.children())) for g in V.default_split(net, body)] == [11, 11]

    class Data:
        sz = (107, 107)
    body = V.default_cut(vmods.inceptionv4())                              # real tensors: with a GPU present _num_features runs the body
    assert [m for m in body.modules() if isinstance(m, torch.nn.BatchNorm2d)][-1].num_features == 256
    assert body.num_features == 1536 and V._num_features(body, Data()) == 1536
