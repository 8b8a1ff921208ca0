"""SENet family without a GPU: state_dict keys and shapes against the reference's (golden g24_senet_keys.json, written by
tools/gen_golden_senet.py), cut / split / feature count, module and argument checks, the ceil-mode output-size rule."""
import json
import os
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import senet, vmods
from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipConv2d, HipGroupedConv2d, HipMaxPool2d

FACTORIES = ['senet154', 'se_resnet50', 'se_resnet101', 'se_resnet152', 'se_resnext50_32x4d', 'se_resnext101_32x4d']


@pytest.mark.parametrize('name', FACTORIES)
def test_state_dict_keys_and_shapes_are_the_references(name):
    with open(os.path.join(GOLDEN, 'g24_senet_keys.json')) as f:
        want = json.load(f)[name]
    with torch.device('meta'):
        net = getattr(vmods, name)()
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == want
    assert isinstance(net, vmods.SENet) and vmods.SENet is senet.SENet


def test_reference_keyed_state_dict_loads_strictly():
    with open(os.path.join(GOLDEN, 'g24_senet_keys.json')) as f:
        want = json.load(f)['se_resnext50_32x4d']
    sd = {k: torch.full(shape, 0.5) if shape else torch.tensor(3) for k, shape in want}
    net = vmods.se_resnext50_32x4d()
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    conv2 = net.layer1[0].conv2
    assert float(conv2.weight.detach().min()) == 0.5 and conv2.weight.is_contiguous(memory_format=torch.channels_last)


def test_layers_run_where_the_design_says():
    with torch.device('meta'):
        x50, s154, r50 = vmods.se_resnext50_32x4d(), vmods.senet154(), vmods.se_resnet50()
    for net, groups in ((x50, 32), (s154, 64)):
        grouped = [m for m in net.modules() if isinstance(m, nn.Conv2d) and m.groups != 1]
        assert grouped and all(type(m) is HipGroupedConv2d and m.groups == groups and m.kernel_size == (3, 3) for m in grouped)
        assert all(m.weight.stride() == (9 * m.weight.shape[1], 1, 3 * m.weight.shape[1], m.weight.shape[1]) for m in grouped if m.weight.shape[1] > 1)
    assert not [m for m in r50.modules() if isinstance(m, HipGroupedConv2d)]                       # groups == 1: plain HipConv2d
    assert all(isinstance(b.conv2, HipConv2d) for b in r50.layer3)
    assert isinstance(s154.layer2[0].downsample[0], HipConv2d) and s154.layer2[0].downsample[0].kernel_size == (3, 3)
    assert isinstance(s154.layer0.pool, HipMaxPool2d) and s154.layer0.pool.ceil_mode
    assert [k for k, _ in s154.layer0.named_children()] == ['conv1', 'bn1', 'relu1', 'conv2', 'bn2', 'relu2', 'conv3', 'bn3', 'relu3', 'pool']
    assert isinstance(s154.dropout, nn.Dropout) and s154.dropout.p == 0.2 and x50.dropout is None


def test_grouped_module_stays_out_of_the_prepared_filter_window():
    assert not hasattr(HipGroupedConv2d, 'nnl_hip_conv') and not hasattr(HipGroupedConv2d(8, 8, 3, groups=2), 'nnl_hip_conv')
    net = senet.SENet(senet.SEResNeXtBottleneck, [1, 1, 1, 1], groups=32, reduction=16, dropout_p=None, inplanes=64, input_3x3=False,
                      downsample_kernel_size=1, downsample_padding=0, num_classes=5)
    mods = ops._Filters(net).mods
    assert mods and not [m for m in mods if isinstance(m, HipGroupedConv2d) or m.groups != 1]
    assert not [m for m in mods if isinstance(m, senet._SEFc)]


def test_cut_split_and_feature_count():
    with torch.device('meta'):
        arch = vmods.se_resnext50_32x4d()
    body = V.default_cut(arch)
    assert len(list(body.children())) == 5
    assert [len(list(g.children())) for g in V.default_split(arch, body)] == [3, 2]
    data = types.SimpleNamespace(sz=(64, 64), categories={i: str(i) for i in range(5)}, bs=2, target_type='single_label')
    if not torch.cuda.is_available():
        assert V._num_features(body, data) == 2048                   # fc2 of the last block: planes * 4
        net = V.ImageClassificationNet(data, vmods.se_resnext50_32x4d())
        assert len(net.layer_groups) == 3 and len(net.param_groups) == 6
        assert next(p for p in net.head.parameters() if p.dim() == 2).shape[1] == 2 * 2048


def test_pretrained_imagenet_raises_and_default_is_none():
    for name in FACTORIES:
        with pytest.raises(RuntimeError, match='never downloads'):
            getattr(vmods, name)(pretrained='imagenet')
    with pytest.raises(RuntimeError, match='load_state_dict'):
        vmods.senet154(num_classes=10, pretrained='imagenet')


def test_domain_violations_name_the_argument():
    x = torch.zeros(1, 8, 6, 6)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        HipGroupedConv2d(8, 8, 5, padding=2, groups=2)(x)
    with pytest.raises(NotImplementedError, match='dilation'):
        HipGroupedConv2d(8, 8, 3, padding=2, dilation=2, groups=2)(x)
    with pytest.raises(NotImplementedError, match='groups'):
        ops.grouped_conv2d(x, torch.zeros(6, 2, 3, 3), None, 1, 1, 4)          # 4 does not divide K = 6
    with pytest.raises(NotImplementedError, match='stride'):
        HipGroupedConv2d(8, 8, 3, stride=3, padding=1, groups=2)(x)
    with pytest.raises(NotImplementedError, match='padding'):
        HipGroupedConv2d(8, 8, 3, padding=2, groups=2)(x)
    with pytest.raises(NotImplementedError, match='padding'):
        HipGroupedConv2d(8, 8, 1, padding=1, groups=2)(x)


def test_library_refuses_what_lies_outside_the_domain():
    "the C entry points return the invalid-argument status before any launch (no GPU needed)"
    from neuralnetworklibrary_amd._lib import lib
    for bad in (dict(R=5), dict(stride=3), dict(pad=2), dict(G=3), dict(R=1, pad=1)):
        a = dict(N=1, H=6, W=6, C=8, K=8, G=2, R=3, stride=1, pad=1)
        a.update(bad)
        assert lib.nnl_gconv2d_fwd(None, None, None, None, a['N'], a['H'], a['W'], a['C'], a['K'], a['G'], a['R'], a['stride'], a['pad'], 0, None) == -1, bad
        assert b'gconv2d_fwd' in lib.nnl_last_error()


@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('H', [7, 8, 15, 16, 112])
def test_ceil_mode_output_size_rule(H, pad):
    want = F.max_pool2d(torch.zeros(1, 1, H, H), 3, 2, pad, ceil_mode=True).shape[-1]
    assert ops.pool_out_size(H, 3, 2, pad, ceil_mode=True) == want
    assert ops.pool_out_size(H, 3, 2, pad) == F.max_pool2d(torch.zeros(1, 1, H, H), 3, 2, pad).shape[-1]
