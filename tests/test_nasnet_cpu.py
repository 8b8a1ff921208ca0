"""NASNet-A-Large without a GPU: state_dict keys / shapes and parameter order against golden G27 (tools/gen_golden_nasnet.py: the real
reference under torch.device('meta')), the zero-pad folding of ops.fold_zero_pad against the literal pad -> op -> slice composition,
the domain checks of the new ops (raised before any device is needed), and the host logic of the registry."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden
from tools.gen_golden_nasnet import FILTERS, NCLS, PARTS, STEM, cell_cases, full_net, short_net

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import nasnet, vmods

# every (R, stride, pad, z) that a folded op of NASNet uses: BranchSeparablesReduction 5x5 / 7x7 at stride 2 and 3x3 at stride 1 (z = 1),
# MaxPoolPad / AvgPoolPad 3x3 at stride 2
FOLDS = [(5, 2, 2, 1), (7, 2, 3, 1), (3, 1, 1, 1), (3, 2, 1, 1)]


@pytest.fixture(scope='module')
def g27():
    out = {}
    for part in PARTS:
        out.update(load_golden(part))
    return out


def test_state_dict_keys_and_shapes_are_the_reference():
    with open(os.path.join(GOLDEN, 'g27_nasnet_keys.json')) as f:
        want = json.load(f)['nasnetalarge']
    with torch.device('meta'):
        net = vmods.nasnetalarge()
    assert isinstance(net, vmods.NASNetALarge) and net.last_linear.out_features == 1000
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == want
    # named_parameters order = state_dict order without the buffers
    buffers = ('running_mean', 'running_var', 'num_batches_tracked')
    assert [n for n, _ in net.named_parameters()] == [k for k, _ in want if not k.endswith(buffers)]


def test_parameter_names_of_the_golden_cases(g27):
    for name, (make, _) in cell_cases(nasnet).items():
        assert [n for n, _ in make().named_parameters()] == [str(s) for s in g27['cell.%s.param_names' % name]], name
    assert [n for n, _ in short_net(nasnet)().named_parameters()] == [str(s) for s in g27['short.param_names']]


@pytest.mark.parametrize('R,stride,pad,z', FOLDS)
def test_fold_zero_pad_is_the_literal_composition(R, stride, pad, z):
    w = torch.arange(1.0, R * R + 1).reshape(1, 1, R, R)
    for H in range(1, 51):
        lo, P = ops.fold_zero_pad(H, R, stride, pad, z)
        assert P == (H + z + 2 * pad - R) // stride + 1 - 1 and lo == pad + z - stride
        if P < 1:
            continue
        assert 0 <= lo <= R - 1 and (P - 1) * stride - lo <= H - 1, 'a folded window misses the image'
        x = torch.arange(1.0, H * H + 1).reshape(1, 1, H, H).double()
        literal = F.conv2d(F.pad(x, (z, 0, z, 0)), w.double(), None, stride, pad)[:, :, 1:, 1:]
        assert literal.shape[2] == P, 'H = %d' % H
        hi = max(0, (P - 1) * stride - lo + R - H)                          # zeros below / right of the image that the last window reaches
        folded = F.conv2d(F.pad(x, (lo, hi, lo, hi)), w.double(), None, stride, 0)[:, :, :P, :P]
        assert torch.equal(literal, folded), 'H = %d' % H
    if (R, stride, pad, z) == (3, 1, 1, 1):
        assert ops.fold_zero_pad(17, R, stride, pad, z) == (1, 17)          # degenerates to the plain convolution
    if (R, stride, pad, z) == (3, 2, 1, 1):
        for H in range(2, 51):                                              # MaxPoolPad: the pad-0 ceil-mode pool has the same windows
            assert ops.fold_zero_pad(H, 3, 2, 1, 1) == (0, ops.pool_out_size(H, 3, 2, 0, ceil_mode=True)) == (0, H // 2)


def test_domain_checks_name_the_argument_before_any_device():
    x, w = torch.zeros(1, 6, 9, 9), torch.zeros(6, 1, 3, 3)
    for match, call in [
            ('kernel_size', lambda: ops.depthwise_conv2d(x, torch.zeros(6, 1, 4, 4), None, 1, 1)),
            ('kernel_size', lambda: ops.depthwise_conv2d(x, torch.zeros(6, 1, 3, 5), None, 1, 1)),
            ('kernel_size', lambda: ops.depthwise_conv2d(x, torch.zeros(6, 1, 9, 9), None, 1, 4)),
            ('stride', lambda: ops.depthwise_conv2d(x, w, None, 3, 1)),
            ('padding', lambda: ops.depthwise_conv2d(x, w, None, 1, 2)),
            ('pad_lo', lambda: ops.depthwise_conv2d(x, w, None, 2, 1, pad_lo=3, out_size=4)),
            ('out_size', lambda: ops.depthwise_conv2d(x, w, None, 2, 1, pad_lo=0, out_size=6)),
            ('depthwise', lambda: ops.depthwise_conv2d(x, torch.zeros(6, 2, 3, 3), None, 1, 1)),
            ('depthwise', lambda: ops.depthwise_conv2d(x, torch.zeros(12, 1, 3, 3), None, 1, 1)),
            ('kernel_size', lambda: ops.avgpool2d(x, 16, 1, 0)),
            ('stride', lambda: ops.avgpool2d(x, 3, 0, 1)),
            ('padding', lambda: ops.avgpool2d(x, 3, 1, 2)),
            ('out_size', lambda: ops.avgpool2d(x, 3, 2, 1, pad_lo=0, out_size=(4, 6))),
            ('stride', lambda: ops.subsample2d(x, 0, 0)),
            ('off', lambda: ops.subsample2d(x, 2, 2)),
            ('4-D', lambda: ops.subsample2d(x[0], 2, 0))]:
        with pytest.raises(NotImplementedError, match=match):
            call()
    conv = nasnet.HipDepthwiseConv2d(6, 6, 3, padding=1, groups=3)
    with pytest.raises(NotImplementedError, match='groups'):
        conv(x)
    with pytest.raises(NotImplementedError, match='dilation'):
        nasnet.HipDepthwiseConv2d(6, 6, 3, padding=2, dilation=2, groups=6)(x)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        nasnet.HipDepthwiseConv2d(6, 6, (3, 5), padding=1, groups=6)(x)


def test_registry_factory_and_feature_count():
    with pytest.raises(RuntimeError, match='never downloads'):
        vmods.nasnetalarge(pretrained='imagenet')
    net = full_net(nasnet)()
    assert net.num_features == 24 * FILTERS and net.last_linear.in_features == 24 * FILTERS and net.last_linear.out_features == NCLS
    assert V.default_cut(net) is net and V.default_split(net, net) == [net]

    class Data:
        sz = (76, 76)
    assert V._num_features(net, Data()) == 24 * FILTERS                    # (the last BatchNorm has 4 * FILTERS channels)
    assert net.cell_stem_0.conv_1x1.conv.in_channels == STEM
