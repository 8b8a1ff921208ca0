"""InceptionResNetV2 without a GPU: state_dict keys / shapes and parameter order against golden G30 (tools/gen_golden_incres.py: the real
reference under torch.device('meta')), the blocks' constants, the domain checks of ops.cat_conv1x1_residual (raised before any device is
needed) and the host logic of the registry."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import inceptionresnetv2 as irn, vmods
from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipConv2d, HipLineConv2d


def test_state_dict_keys_shapes_and_block_constants_are_the_reference():
    with open(os.path.join(GOLDEN, 'g30_incres_keys.json')) as f:
        want = json.load(f)['inceptionresnetv2']
    with torch.device('meta'):
        net = vmods.inceptionresnetv2()
    assert isinstance(net, vmods.InceptionResNetV2) and net.last_linear.out_features == 1000 and net.input_size == (299, 299, 3)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want
    buffers = ('running_mean', 'running_var', 'num_batches_tracked')
    assert [n for n, _ in net.named_parameters()] == [k for k, _ in want if not k.endswith(buffers)]
    blocks = [m for m in net.modules() if isinstance(m, (irn.Block35, irn.Block17, irn.Block8))]
    assert [(type(m).__name__, m.scale, m.noReLU) for m in blocks] == \
        [('Block35', 0.17, False)] * 10 + [('Block17', 0.10, False)] * 20 + [('Block8', 0.20, False)] * 9 + [('Block8', 1.0, True)]
    assert all(isinstance(m.conv2d, HipConv2d) and m.conv2d.kernel_size == (1, 1) and m.conv2d.bias is not None for m in blocks)
    convs = [m.conv for m in net.modules() if isinstance(m, irn.BasicConv2d)]
    assert len(convs) == 204 and sum(isinstance(c, HipLineConv2d) for c in convs) == 60
    assert all(isinstance(c, HipConv2d) == (c.kernel_size[0] == c.kernel_size[1]) for c in convs)
    assert all(m.bn.eps == 0.001 for m in net.modules() if isinstance(m, irn.BasicConv2d))


def test_domain_checks_name_the_argument_before_any_device():
    z = torch.zeros
    for match, call in [
            ('sources', lambda: ops.cat_conv1x1_residual([], z(8, 8, 1, 1), None, None)),
            ('sources', lambda: ops.cat_conv1x1_residual([z(1, 4, 3, 3)] * 5, z(8, 20, 1, 1), None, None)),
            ('sources', lambda: ops.cat_conv1x1_residual([z(1, 6, 3, 3)], z(8, 6, 1, 1), None, None)),
            ('sources', lambda: ops.cat_conv1x1_residual([z(1, 260, 3, 3)] * 2, z(8, 520, 1, 1), None, None)),
            ('sources', lambda: ops.cat_conv1x1_residual([z(1, 4, 3, 3), z(1, 4, 3, 2)], z(8, 8, 1, 1), None, None)),
            ('weight', lambda: ops.cat_conv1x1_residual([z(1, 4, 3, 3)] * 2, z(8, 4, 1, 1), None, None)),
            ('weight', lambda: ops.cat_conv1x1_residual([z(1, 8, 3, 3)], z(8, 8, 3, 3), None, None)),
            ('out_channels', lambda: ops.cat_conv1x1_residual([z(1, 8, 3, 3)], z(6, 8, 1, 1), None, None)),
            ('bias', lambda: ops.cat_conv1x1_residual([z(1, 8, 3, 3)], z(8, 8, 1, 1), z(4), None)),
            ('residual', lambda: ops.cat_conv1x1_residual([z(1, 8, 3, 3)], z(8, 8, 1, 1), None, z(1, 4, 3, 3)))]:
        with pytest.raises(NotImplementedError, match=match):
            call()


def test_registry_factory_cut_split_and_feature_count():
    for pretrained in ('imagenet', 'imagenet+background'):
        with pytest.raises(RuntimeError, match='never downloads'):
            vmods.inceptionresnetv2(pretrained=pretrained)
    with torch.device('meta'):
        net = vmods.inceptionresnetv2(num_classes=7)
    assert net.last_linear.out_features == 7
    body = V.default_cut(net)
    assert body is net and V.default_split(net, body) == [net]
    assert net.num_features == 1536 and net.conv2d_7b.bn.num_features == 1536
