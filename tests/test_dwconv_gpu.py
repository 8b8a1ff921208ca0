"""K18 kernels — depthwise convolution (csrc/dwconv.hip), average pool, strided subsample and the scalar-channel max-pool route
(csrc/pool.hip) — through ops.* and the C entries, against fp64 torch on the CPU: F.conv2d(groups=C), F.avg_pool2d, and the literal
F.pad + slice compositions for the folded ("pad top/left, op at stride 2, drop the first row and column") forms.

Tolerances are derived, not tuned: per output, n 2^-24 sum|terms|, the sum of absolute terms taken from an fp64 run of the same
composition on |operands| (n accumulations, each rounding to nearest once: a relative error of at most 2^-24 of the running sum, which
never exceeds sum|terms|).  n = R^2 + 1 for forward / dgrad, k^2 + 1 for pooling, N P Q + 1 for wgrad and the bias gradient.  The
subsample copies: exact.  The worst ratio is printed before it is asserted.  Every forward, dgrad and wgrad runs twice: torch.equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
MAPS = [(5, 7), (10, 10), (19, 13)]
CS = [6, 16, 70]


def bounded(what, got, ref, terms, n):
    got, ref, terms = (t.detach().cpu().double().numpy() for t in (got, ref, terms))
    assert got.shape == ref.shape, '%s: shape %s vs %s' % (what, got.shape, ref.shape)
    err, allowed = np.abs(got - ref), n * U * terms
    exact = allowed == 0
    assert np.all(err[exact] == 0), '%s: a sum without terms is not exactly zero' % what
    worst = float(np.max(err[~exact] / allowed[~exact])) if (~exact).any() else 0.0
    print('%-28s worst |hip - f64| / (n u sum|terms|) = %.3f   (n = %d)' % (what, worst, n))
    assert worst <= 1.0, '%s: off the fp64 reference by %.3f of the derived bound' % (what, worst)


def _inputs(N, C, H, W, R, seed, bias):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    x[torch.rand(N, C, H, W, generator=g) < 0.2] = 0.0                    # exact zeros next to negative values: the ReLU gate's edge
    w = torch.randn(C, 1, R, R, generator=g) / R
    b = torch.randn(C, generator=g) if bias else None
    return x, w, b


def _ref_conv(x, w, b, R, stride, mode, relu_in):
    "the literal composition in whatever dtype the operands have"
    a = torch.relu(x) if relu_in else x
    C, p = x.shape[1], R // 2
    if mode == 'fold':                                                    # nasnet.py:158-162
        return F.conv2d(F.pad(a, (1, 0, 1, 0)), w, b, stride, p, 1, C)[:, :, 1:, 1:]
    y = F.conv2d(a, w, b, stride, p, 1, C)
    return y[:, :, :1, :1] if mode == 'one' else y


def _conv_cases():
    cases, i = [], 0
    for sweep in range(2):
        for R in (3, 5, 7):
            for stride in (1, 2):
                for mode in ('sym', 'fold'):
                    H, W = MAPS[(i + sweep) % 3]
                    cases.append((1 + 2 * ((i // 2 + sweep) % 2), CS[(i // 2 + 2 * sweep) % 3], H, W, R, stride, mode, bool((i + sweep) % 2),
                                  bool((i // 3) % 2)))
                    i += 1
    cases.append((1, 6, 5, 7, 7, 2, 'one', True, True))                   # P = Q = 1 on a map smaller than the window
    cases.append((3, 70, 10, 10, 5, 2, 'one', False, False))
    return cases


@pytest.mark.parametrize('N,C,H,W,R,stride,mode,relu_in,bias', _conv_cases(),
                         ids=lambda v: str(int(v)) if isinstance(v, (bool, int)) else str(v))
def test_depthwise_conv2d_forward_and_gradients(N, C, H, W, R, stride, mode, relu_in, bias):
    x, w, b = _inputs(N, C, H, W, R, 1000 * R + 10 * C + H + stride, bias)
    p = R // 2
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    ref = _ref_conv(xr, wr, br, R, stride, mode, relu_in)
    dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7))
    ref.backward(dy.double())
    # sum of |terms| per output / per gradient entry: the same composition on absolute operands (no gate: a bound)
    xa = (torch.relu(x) if relu_in else x).abs().double().requires_grad_(True)
    wa, ba = w.abs().double().requires_grad_(True), (b.abs().double().requires_grad_(True) if bias else None)
    ta = _ref_conv(xa, wa, ba, R, stride, mode, False)
    ta.backward(dy.abs().double())

    if mode == 'sym':
        kw = {}
    elif mode == 'fold':
        (lo, P), (_, Q) = ops.fold_zero_pad(H, R, stride, p, 1), ops.fold_zero_pad(W, R, stride, p, 1)
        assert lo == (p - 1 if stride == 2 else p)
        kw = dict(pad_lo=lo, out_size=(P, Q))
    else:
        kw = dict(pad_lo=p, out_size=1)
    runs = []
    for _ in range(2):
        xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        bg = b.to(DEV).requires_grad_(True) if bias else None
        y = ops.depthwise_conv2d(xg, wg, bg, stride, p, relu_in=relu_in, **kw)
        y.backward(dy.to(DEV))
        runs.append((y.detach(), xg.grad, wg.grad) + ((bg.grad,) if bias else ()))
    assert all(torch.equal(a, c) for a, c in zip(*runs)), 'two calls on the same inputs differ'
    y, dx, dw = runs[0][:3]
    npq = N * ref.shape[2] * ref.shape[3]
    bounded('forward', y, ref, ta, R * R + 1)
    bounded('dgrad', dx, xr.grad, xa.grad, R * R + 1)
    bounded('wgrad', dw, wr.grad, wa.grad, npq + 1)
    if relu_in:
        assert bool((dx.cpu()[x <= 0] == 0).all()), 'gate: dx is not zero where x <= 0'
    if bias:
        bounded('bias grad', runs[0][3], br.grad, dy.abs().double().sum((0, 2, 3)), npq + 1)


def test_wgrad_adds_slabs_in_a_fixed_order():
    "a shape that needs more than one slab (the threshold is read from the workspace query), straight through the C entries"
    N, C, H, W, R = 3, 70, 19, 13, 5
    x, w, _ = _inputs(N, C, H, W, R, 5, False)
    dims = (N, H, W, C, H, W, R, 1, 2)
    wsb = int(lib.nnl_dwconv2d_wgrad_workspace_bytes(*dims))
    assert wsb >= 2 * C * R * R * 4 and wsb % (C * R * R * 4) == 0, 'workspace %d B: fewer than two slabs' % wsb
    assert int(lib.nnl_dwconv2d_wgrad_workspace_bytes(1, 5, 7, C, 5, 7, R, 1, 2)) == 0, 'a 35-pixel problem is one slab'
    dy = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(8))
    xn, dyn = (t.permute(0, 2, 3, 1).contiguous().to(DEV) for t in (x, dy))
    outs = []
    for _ in range(2):
        dw = torch.empty(C, 1, R, R, device=DEV)
        ws = torch.empty(wsb // 4, device=DEV)
        assert lib.nnl_dwconv2d_wgrad(ptr(xn), ptr(dyn), ptr(dw), ptr(ws), wsb, *dims, 0, None) == 0
        outs.append(dw)
    assert torch.equal(*outs)
    assert lib.nnl_dwconv2d_wgrad(ptr(xn), ptr(dyn), ptr(outs[0]), ptr(ws), wsb - 4, *dims, 0, None) != 0, 'short workspace accepted'
    wr = w.double().requires_grad_(True)
    F.conv2d(x.double(), wr, None, 1, 2, 1, C).backward(dy.double())
    wa = w.abs().double().requires_grad_(True)
    F.conv2d(x.abs().double(), wa, None, 1, 2, 1, C).backward(dy.abs().double())
    bounded('wgrad, %d slabs' % (wsb // (C * R * R * 4)), outs[0], wr.grad, wa.grad, N * H * W + 1)


def test_bad_arguments_are_errors_from_c_without_a_launch():
    N, C, H, W, R = 1, 6, 10, 10, 3
    x = torch.zeros(N, H, W, C, device=DEV)
    w = torch.zeros(C, 1, R, R, device=DEV)
    y = torch.full((N, 8, 8, C), 7.0, device=DEV)
    ok = (N, H, W, C, 5, 5, R, 2, 1)                                      # the symmetric 3x3 / stride 2 / pad 1: P = 5

    def fwd(dims, px=x, pw=w, py=y):
        return lib.nnl_dwconv2d_fwd(ptr(px), ptr(pw), None, ptr(py), *dims, 0, None)
    assert fwd(ok) == 0
    torch.cuda.synchronize()
    y.fill_(7.0)
    bad = {'P one too large': (N, H, W, C, 7, 5, R, 2, 1),               # (7 - 1) 2 - 1 = 11 > H - 1: the window misses the image
           'Q one too large': (N, H, W, C, 5, 7, R, 2, 1),
           'pad_lo = R': (N, H, W, C, 5, 5, R, 2, R),
           'R = 4': (N, H, W, C, 5, 5, 4, 2, 1),
           'stride 3': (N, H, W, C, 3, 3, R, 3, 1),
           'P = 0': (N, H, W, C, 0, 5, R, 2, 1)}
    for what, dims in bad.items():
        assert fwd(dims) != 0, what
        assert int(lib.nnl_dwconv2d_wgrad_workspace_bytes(*dims)) == 0, what
        assert lib.nnl_dwconv2d_dgrad(ptr(y), ptr(w), None, ptr(x), *dims, 0, None) != 0, what
        assert lib.nnl_dwconv2d_wgrad(ptr(x), ptr(y), ptr(w), None, 0, *dims, 0, None) != 0, what
        if what not in ('R = 4', 'stride 3'):                            # (both are windows the average pool takes)
            assert lib.nnl_avgpool2d_fwd(ptr(x), ptr(y), *dims, 0, None) != 0, what
            assert lib.nnl_avgpool2d_bwd(ptr(y), ptr(x), *dims, 0, None) != 0, what
    assert fwd(ok, px=None) != 0 and fwd(ok, pw=None) != 0 and fwd(ok, py=None) != 0, 'null pointer'
    assert lib.nnl_dwconv2d_dgrad(None, ptr(w), None, ptr(x), *ok, 0, None) != 0
    assert lib.nnl_dwconv2d_dgrad(ptr(y), ptr(w), None, ptr(x), *ok, 1, None) != 0, 'relu_in without x'
    assert lib.nnl_dwconv2d_wgrad(ptr(x), None, ptr(w), None, 0, *ok, 0, None) != 0
    assert lib.nnl_avgpool2d_fwd(None, ptr(y), N, H, W, C, 5, 5, 3, 2, 1, 0, None) != 0
    assert lib.nnl_avgpool2d_bwd(ptr(y), None, N, H, W, C, 5, 5, 3, 2, 1, 0, None) != 0
    assert lib.nnl_avgpool2d_fwd(ptr(x), ptr(y), N, H, W, C, 5, 5, 16, 2, 1, 0, None) != 0, 'ksize 16'
    assert lib.nnl_subsample2d_fwd(None, ptr(y), N, H, W, C, 5, 5, 2, 0, None) != 0
    assert lib.nnl_subsample2d_bwd(ptr(y), ptr(x), N, H, W, C, 5, 5, 0, 0, None) != 0, 'stride 0'
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), 'a refused call wrote its output'


def _ref_avgpool(x, k, stride, pad, cip, zero_pad):
    if zero_pad:                                                          # AvgPoolPad, nasnet.py:86-90
        return F.avg_pool2d(F.pad(x, (1, 0, 1, 0)), k, stride, pad, count_include_pad=cip)[:, :, 1:, 1:]
    return F.avg_pool2d(x, k, stride, pad, count_include_pad=cip)


@pytest.mark.parametrize('C', [6, 16])
@pytest.mark.parametrize('H,W,k,stride,pad,cip,zero_pad', [
    (19, 13, 3, 1, 1, False, False), (19, 13, 3, 1, 1, True, False), (10, 10, 3, 2, 1, False, False), (19, 13, 3, 2, 1, True, False),
    (10, 10, 3, 2, 1, False, True), (19, 13, 3, 2, 1, False, True), (11, 11, 11, 1, 0, True, False), (5, 7, 3, 2, 1, False, False)])
def test_avgpool2d(C, H, W, k, stride, pad, cip, zero_pad):
    N = 3
    x, _, _ = _inputs(N, C, H, W, 3, 31 * C + H + k, False)
    xr = x.double().requires_grad_(True)
    ref = _ref_avgpool(xr, k, stride, pad, cip, zero_pad)
    dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(9))
    ref.backward(dy.double())
    xa = x.abs().double().requires_grad_(True)
    ta = _ref_avgpool(xa, k, stride, pad, cip, zero_pad)
    ta.backward(dy.abs().double())
    kw = {}
    if zero_pad:
        (lo, P), (_, Q) = ops.fold_zero_pad(H, k, stride, pad, 1), ops.fold_zero_pad(W, k, stride, pad, 1)
        kw = dict(pad_lo=lo, out_size=(P, Q))
    runs = []
    for _ in range(2):
        xg = x.to(DEV).requires_grad_(True)
        y = ops.avgpool2d(xg, k, stride, pad, count_include_pad=cip, **kw)
        y.backward(dy.to(DEV))
        runs.append((y.detach(), xg.grad))
    assert all(torch.equal(a, c) for a, c in zip(*runs))
    bounded('avgpool forward', runs[0][0], ref, ta, k * k + 1)
    bounded('avgpool backward', runs[0][1], xr.grad, xa.grad, k * k + 1)


@pytest.mark.parametrize('C', [6, 16])
@pytest.mark.parametrize('H,W', [(10, 10), (19, 13), (5, 7)])
@pytest.mark.parametrize('off', [0, 1])
def test_subsample2d_is_exact(C, H, W, off):
    x, _, _ = _inputs(2, C, H, W, 3, H + off, False)
    xc = x.clone().requires_grad_(True)
    ref = F.avg_pool2d(F.pad(xc, (0, 1, 0, 1))[:, :, 1:, 1:] if off else xc, 1, 2, count_include_pad=False)     # nasnet.py:232-238, 263-266
    dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(10))
    ref.backward(dy)
    xg = x.to(DEV).requires_grad_(True)
    y = ops.subsample2d(xg, 2, off)
    y.backward(dy.to(DEV))
    assert torch.equal(y.cpu(), ref) and torch.equal(xg.grad.cpu(), xc.grad)


@pytest.mark.parametrize('H,W,k,s,p,ceil', [(19, 13, 3, 2, 1, False), (10, 10, 3, 2, 0, True), (5, 7, 3, 2, 0, True), (9, 10, 3, 1, 1, False)])
def test_maxpool2d_scalar_channel_route_with_ties(H, W, k, s, p, ceil):
    "C = 6: the route for C % 4 != 0; ties (quantised, rectified input) go to the first maximum, as on the vector route and in torch"
    g = torch.Generator().manual_seed(H)
    x = (torch.randn(3, 6, H, W, generator=g) * 2).round().clamp_(min=0) / 2
    xc = x.clone().requires_grad_(True)
    ref = F.max_pool2d(xc, k, s, p, ceil_mode=ceil)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    xg = x.to(DEV).requires_grad_(True)
    y = ops.maxpool2d(xg, k, s, p, ceil_mode=ceil)
    y.backward(dy.to(DEV))
    assert torch.equal(y.cpu(), ref)
    # a pixel collects at most ceil(k / s)^2 values of dy: n = that + 1, terms = the same backward on |dy|
    xa = x.clone().requires_grad_(True)
    F.max_pool2d(xa, k, s, p, ceil_mode=ceil).backward(dy.abs())
    bounded('maxpool backward', xg.grad, xc.grad, xa.grad, (-(-k // s)) ** 2 + 1)
    if ceil:                                                              # MaxPoolPad (nasnet.py:65-76) is this pool
        pad_form = F.max_pool2d(F.pad(x, (1, 0, 1, 0)), 3, 2, 1)[:, :, 1:, 1:]
        assert torch.equal(y.cpu(), pad_form)
