"""ResNeXt-101 without a GPU: the module tree against golden G29's key file, the factories' arguments, default_cut / default_split."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import vmods
from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipGroupedConv2d

NAMES = ['resnext101_32x4d', 'resnext101_64x4d']


def meta(name, **kw):
    with torch.device('meta'):
        return getattr(vmods, name)(**kw)


@pytest.mark.parametrize('name', NAMES)
def test_keys_shapes_and_parameter_order_are_the_reference_s(name):
    with open(os.path.join(GOLDEN, 'g29_resnext_keys.json')) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)[name]]
    net = meta(name)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    params = [k for k, _ in want if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    assert [k for k, _ in net.named_parameters()] == params
    net.load_state_dict({k: torch.empty(s, device='meta') for k, s in want}, strict=True)


@pytest.mark.parametrize('name', NAMES)
def test_grouped_convolutions_cut_and_split(name):
    net = meta(name, num_classes=7)
    assert net.last_linear.out_features == 7 and isinstance(net, getattr(vmods, 'ResNeXt101_' + name[-5:]))
    gconvs = [m for m in net.modules() if isinstance(m, HipGroupedConv2d)]
    assert len(gconvs) == 33 and sum(m.in_channels // m.groups in (16, 32) for m in gconvs) == 26
    body = V.default_cut(net)
    assert body is net.features
    groups = V.default_split(net, body)
    assert [len(g) for g in groups] == [6, 2] and groups[1][0] is net.features[6]


def test_factories_never_download_and_share_nothing():
    for name in NAMES:
        with pytest.raises(RuntimeError, match='never downloads'):
            getattr(vmods, name)(pretrained='imagenet')
    a, b = meta(NAMES[0]), meta(NAMES[0])
    assert a.features is not b.features
    assert not {id(p) for p in a.parameters()} & {id(p) for p in b.parameters()}
