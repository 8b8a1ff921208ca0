"""GPU parity of the fused BatchNorm(+residual)(+ReLU) kernels against torch CPU BatchNorm."""
import os

import pytest
import torch
import torch.nn as nn

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = [  # shape, residual, relu, training, mean offset
    ((4, 64, 14, 14), True, True, True, 0.0),
    ((2, 128, 7, 9), False, True, True, 3.0),
    ((3, 512, 2, 2), True, False, True, 0.0),
    ((64, 14), False, False, True, 50.0),          # BatchNorm1d, C % 4 != 0, |mean| >> std (cancellation check)
    ((1024, 1000), False, False, True, 0.0),       # tabular hidden layer
    ((8, 1024), False, False, True, 0.0),
    ((4, 64, 14, 14), True, True, False, 0.0),     # eval mode (frozen BN)
    ((5, 20, 3, 3), False, True, False, 1.0),
    ((8, 64, 56, 56), True, True, True, 0.5),      # ResNet-34 stages at 8 images per GPU (the strong-scaling regime)
    ((8, 512, 7, 7), True, True, True, 0.0),
    ((16, 256, 14, 14), False, True, True, 2.0),
    ((2, 2048, 4, 4), True, True, True, 0.0),      # ResNet-50's widest layer
]


@pytest.mark.parametrize('case', CASES, ids=[str(c) for c in CASES])
def test_bn_act(case):
    from neuralnetworklibrary_amd import ops
    shape, has_res, relu, training, offset = case
    g = torch.Generator().manual_seed(len(shape) * 100 + shape[1])
    C = shape[1]
    x = torch.randn(shape, generator=g) * 1.7 + offset
    res = torch.randn(shape, generator=g) if has_res else None
    dy = torch.randn(shape, generator=g)
    mk = nn.BatchNorm2d if len(shape) == 4 else nn.BatchNorm1d
    bn_c = mk(C)
    with torch.no_grad():
        bn_c.weight.copy_(torch.randn(C, generator=g) * 0.3 + 1)
        bn_c.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn_c.running_mean.copy_(torch.randn(C, generator=g) * 0.1 + offset)
        bn_c.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    bn_g = mk(C)
    bn_g.load_state_dict(bn_c.state_dict())
    bn_g = bn_g.to(DEV)
    bn_c.train(training); bn_g.train(training)

    xc = x.clone().requires_grad_(True)
    rc = res.clone().requires_grad_(True) if has_res else None
    yc = bn_c(xc)
    if has_res:
        yc = yc + rc
    if relu:
        yc = torch.relu(yc)
    yc.backward(dy)

    xg = x.to(DEV).requires_grad_(True)
    rg = res.to(DEV).requires_grad_(True) if has_res else None
    yg = ops.bn_act(bn_g, xg, residual=rg, relu=relu)
    yg.backward(dy.to(DEV))

    assert_close(yg, yc, 1e-4, 1e-5, 'y')
    assert_close(xg.grad, xc.grad, 1e-3, 1e-5 * xc.grad.abs().max().item() + 1e-7, 'dx')
    if has_res:
        assert_close(rg.grad, rc.grad, 1e-5, 1e-6, 'dres')
    assert_close(bn_g.weight.grad, bn_c.weight.grad, 1e-3, 1e-4 * bn_c.weight.grad.abs().max().item(), 'dgamma')
    assert_close(bn_g.bias.grad, bn_c.bias.grad, 1e-3, 1e-4 * bn_c.bias.grad.abs().max().item(), 'dbeta')
    assert_close(bn_g.running_mean, bn_c.running_mean, 1e-5, 1e-5, 'running_mean')
    assert_close(bn_g.running_var, bn_c.running_var, 1e-4, 1e-6, 'running_var')
    assert int(bn_g.num_batches_tracked) == int(bn_c.num_batches_tracked)


@pytest.mark.parametrize('offset', [0.0, 40.0], ids=['centred', 'mean>>std'])
def test_conv_bn_act_epilogue_statistics(offset):
    """ops.conv_bn_act: from a layer's second training step on, the batch statistics come from the convolution's epilogue
    (shifted sums around the previous step's batch mean).  Output, running statistics and all gradients must match
    conv2d -> BatchNorm2d -> +residual in fp64, also when the running mean is useless as a pivot (never updated towards
    a batch mean that sits 20+ sigma away) and when the data mean moves between steps."""
    from neuralnetworklibrary_amd import ops
    from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipConv2d
    g = torch.Generator().manual_seed(11)
    N, Ci, Co, S = 8, 64, 128, 28                       # 6272 output rows: balanced / plain 64x64 tiles with tail rows
    conv = HipConv2d(Ci, Co, 3, stride=1, padding=1, bias=False).to(DEV)
    bn = nn.BatchNorm2d(Co).to(DEV)
    w64 = conv.weight.detach().double().cpu()
    ref_bn = nn.BatchNorm2d(Co).double()
    conv.train(); bn.train(); ref_bn.train()
    for step in range(3):
        x = torch.randn(N, Ci, S, S, generator=g) + offset * (1 + 0.05 * step)
        res = torch.randn(N, Co, S, S, generator=g)
        dy = torch.randn(N, Co, S, S, generator=g)
        xg, rg = x.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True)
        for p in list(conv.parameters()) + list(bn.parameters()):
            p.grad = None
        yg = ops.conv_bn_act(conv, bn, xg, residual=rg, relu=False)   # no ReLU: a gate flipped by rounding would move dx by O(1)
        ops.prepare_backward(torch.nn.Sequential(conv, bn))
        yg.backward(dy.to(DEV))
        ops.finish_backward()
        fused = os.environ.get('NNL_BN_EPI_STATS', '1') != '0'      # (the A/B switch turns the epilogue statistics off)
        assert (getattr(bn, '_nnl_pivot', None) is not None) == fused

        xc, rc = x.double().requires_grad_(True), res.double().requires_grad_(True)
        wc = w64.clone().requires_grad_(True)
        for p in ref_bn.parameters():
            p.grad = None
        yc = ref_bn(torch.nn.functional.conv2d(xc, wc, None, 1, 1)) + rc
        yc.backward(dy.double())
        tag = 'step %d ' % step
        assert_close(yg, yc.float(), 2e-4, 2e-4, tag + 'y')
        assert_close(bn.running_mean, ref_bn.running_mean.float(), 1e-4, 1e-5, tag + 'running_mean')
        assert_close(bn.running_var, ref_bn.running_var.float(), 1e-3, 1e-5, tag + 'running_var')
        if fused:
            assert_close(bn._nnl_pivot, torch.nn.functional.conv2d(xc, wc, None, 1, 1).mean((0, 2, 3)).float(), 1e-4, 1e-4, tag + 'pivot')
        for name, a, b in (('dx', xg.grad, xc.grad), ('dres', rg.grad, rc.grad), ('dw', conv.weight.grad, wc.grad),
                           ('dgamma', bn.weight.grad, ref_bn.weight.grad), ('dbeta', bn.bias.grad, ref_bn.bias.grad)):
            assert_close(a, b.float(), 2e-3, 2e-3 * b.abs().max().item(), tag + name)


# ---- module modes that ops.bn_act accepts, against the torch module in fp64 -------------------------------------------------------------------
def _module_pair(mk, C, g, **kw):
    """the module under test (fp32, on the GPU) and its fp64 twin with the same parameters and buffers"""
    ref = mk(C, **kw).double()
    with torch.no_grad():
        if ref.affine:
            ref.weight.copy_(torch.randn(C, generator=g) * 0.3 + 1)
            ref.bias.copy_(torch.randn(C, generator=g) * 0.3)
        if ref.track_running_stats:
            ref.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
            ref.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    bn = mk(C, **kw)
    bn.load_state_dict(ref.state_dict())
    return bn.to(DEV), ref


def _module_step(bn, ref, x, dy, res, relu, tag):
    from neuralnetworklibrary_amd import ops
    for m in (bn, ref):
        for p in m.parameters():
            p.grad = None
    xc = x.double().detach().requires_grad_(True)
    rc = res.double().requires_grad_(True) if res is not None else None
    yc = ref(xc)
    yc = yc + rc if res is not None else yc
    yc = torch.relu(yc) if relu else yc
    yc.backward(dy.double())
    xg = x.to(DEV).requires_grad_(True)
    rg = res.to(DEV).requires_grad_(True) if res is not None else None
    yg = ops.bn_act(bn, xg, residual=rg, relu=relu)
    yg.backward(dy.to(DEV))
    assert yg.shape == yc.shape
    assert_close(yg, yc, 1e-4, 1e-5, tag + 'y')
    assert_close(xg.grad, xc.grad, 1e-3, 1e-5 * xc.grad.abs().max().item() + 1e-7, tag + 'dx')
    if res is not None:
        assert_close(rg.grad, rc.grad, 1e-5, 1e-6, tag + 'dres')
    if ref.affine:
        assert_close(bn.weight.grad, ref.weight.grad, 1e-3, 1e-4 * ref.weight.grad.abs().max().item(), tag + 'dgamma')
        assert_close(bn.bias.grad, ref.bias.grad, 1e-3, 1e-4 * ref.bias.grad.abs().max().item(), tag + 'dbeta')
    else:
        assert bn.weight is None and bn.bias is None
    if ref.track_running_stats:
        assert_close(bn.running_mean, ref.running_mean, 1e-5, 1e-5, tag + 'running_mean')
        assert_close(bn.running_var, ref.running_var, 1e-4, 1e-6, tag + 'running_var')
        assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked), tag + 'num_batches_tracked'
    else:
        assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None


MODULE_MODES = [  # name, module, input shape, module arguments, training, residual, relu, steps, channels-last input
    ('affine=False', nn.BatchNorm2d, (4, 12, 5, 7), dict(affine=False), True, True, True, 1, False),
    ('affine=False,eval', nn.BatchNorm2d, (4, 12, 5, 7), dict(affine=False), False, False, True, 1, False),
    ('track_running_stats=False,train', nn.BatchNorm2d, (3, 8, 6, 5), dict(track_running_stats=False), True, False, True, 1, False),
    ('track_running_stats=False,eval', nn.BatchNorm2d, (3, 8, 6, 5), dict(track_running_stats=False), False, True, False, 1, False),
    ('momentum=None', nn.BatchNorm2d, (4, 16, 3, 5), dict(momentum=None), True, False, True, 3, False),
    ('momentum=None,1d', nn.BatchNorm1d, (9, 6), dict(momentum=None), True, False, False, 3, False),
    ('[N,C,L]', nn.BatchNorm1d, (5, 12, 7), dict(), True, True, True, 1, False),
    ('[N,C,L],odd C,eval', nn.BatchNorm1d, (5, 7, 3), dict(), False, False, True, 1, False),
    ('C=14,relu,residual', nn.BatchNorm1d, (64, 14), dict(), True, True, True, 1, False),
    ('C=14,relu,residual,2d', nn.BatchNorm2d, (3, 14, 5, 3), dict(), True, True, True, 1, False),
    ('channels-last', nn.BatchNorm2d, (4, 16, 7, 5), dict(), True, True, True, 1, True),
    ('channels-last,eval', nn.BatchNorm2d, (4, 16, 7, 5), dict(), False, False, True, 1, True),
]


@pytest.mark.parametrize('mode', MODULE_MODES, ids=[m[0] for m in MODULE_MODES])
def test_bn_act_module_modes(mode):
    name, mk, shape, kw, training, has_res, relu, steps, channels_last = mode
    g = torch.Generator().manual_seed(sum(shape))
    bn, ref = _module_pair(mk, shape[1], g, **kw)
    bn.train(training); ref.train(training)
    for step in range(steps):
        x = torch.randn(shape, generator=g) * 1.7 + 0.5 * (step + 1)
        res = torch.randn(shape, generator=g) if has_res else None
        dy = torch.randn(shape, generator=g)
        if channels_last:
            x, dy = x.contiguous(memory_format=torch.channels_last), dy.contiguous(memory_format=torch.channels_last)
            res = res.contiguous(memory_format=torch.channels_last) if has_res else None
        _module_step(bn, ref, x, dy, res, relu, '%s step %d ' % (name, step))
