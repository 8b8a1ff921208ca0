"""K19 line convolution (csrc/lineconv.hip) through ops.line_conv2d and the C entries, against fp64 F.conv2d(x, w, b, 1, (0, p) | (p, 0)).

Bound and `bounded` helper of tests/test_dwconv_gpu.py: per value n 2^-24 sum|terms|, the sum from the same fp64 composition on absolute
operands; it holds for any summation order, so the wgrad slabs do not change it.  n = T C + 2 forward, T K + 1 dgrad, N H W + 1 wgrad and
bias gradient.  The worst ratio is printed before it is asserted.  Every case runs twice: torch.equal."""
import pytest
import torch
import torch.nn.functional as F

from test_dwconv_gpu import bounded

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
AX_H, AX_W = 0, 1

# (N, C, K, H, W, T, axis, bias, relu) — what each shape is for, with 64-row x 64-filter tiles and 16-channel chunks:
CASES = [
    (1, 4, 4, 5, 17, 7, AX_W, False, False),       # one partial tile; C and K below a chunk / a tile
    (3, 20, 36, 5, 17, 7, AX_W, True, True),       # 255 rows: tiles end mid-line (64 = 3 x 17 + 13); channel-chunk tail; K-tile tail
    (3, 20, 36, 17, 5, 7, AX_H, True, False),      # the same along H: line (n, w), pixel stride W
    (1, 96, 96, 17, 5, 3, AX_W, False, True),      # lines of 5 under 3 taps; several K tiles; six full chunks
    (3, 96, 36, 5, 17, 3, AX_H, True, True),       # lines of 5 along H
    (1, 20, 96, 3, 75, 7, AX_W, True, False),      # lines longer than a tile (75 > 64): segments with real halos
    (1, 20, 4, 75, 3, 7, AX_H, False, True),       # the same along H
    (3, 4, 36, 3, 75, 3, AX_W, False, False),
    (3, 96, 96, 75, 3, 7, AX_W, True, True),       # lines of 3 under 7 taps: the halo is longer than the line
    (1, 20, 36, 3, 75, 7, AX_H, False, False),     # lines of 3 along H
    (3, 20, 4, 2, 3, 7, AX_W, True, True),         # L = 3 < T, 18 rows
    (1, 4, 96, 2, 3, 7, AX_H, False, False),       # L = 2 < T
    (3, 96, 36, 1, 8, 7, AX_W, False, True),       # an 8-wide map under 7 taps
    (1, 20, 36, 1, 8, 3, AX_H, True, False),       # L = 1 along H
    (3, 20, 96, 8, 1, 7, AX_W, True, True),        # L = 1 along W: every row its own line
    (1, 4, 4, 8, 1, 3, AX_H, False, False),
]


def _case(N, C, K, H, W, T, axis, bias, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn((K, C, T, 1) if axis == AX_H else (K, C, 1, T), generator=g) / (T * C) ** 0.5
    b = torch.randn(K, generator=g) if bias else None
    return x, w, b, ((T // 2, 0) if axis == AX_H else (0, T // 2))


def _reference(x, w, b, pad, relu, dy=None):
    "fp64 output and gradients, and the sums of absolute terms of each from the same composition on absolute operands"
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = None if b is None else b.double().requires_grad_(True)
    pre = F.conv2d(xr, wr, br, 1, pad)
    ref = torch.relu(pre) if relu else pre
    if dy is None:
        dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7))
    ref.backward(dy.double())
    xa, wa = x.abs().double().requires_grad_(True), w.abs().double().requires_grad_(True)
    ba = None if b is None else b.abs().double().requires_grad_(True)
    ta = F.conv2d(xa, wa, ba, 1, pad)
    gate = (pre > 0).double() if relu else 1.0                             # the gradient terms that pass the gate
    ta.backward(dy.abs().double() * gate)
    return dy, ref, (xr.grad, wr.grad, None if b is None else br.grad), ta, (xa.grad, wa.grad, None if b is None else ba.grad)


@pytest.mark.parametrize('N,C,K,H,W,T,axis,bias,relu', CASES, ids=lambda v: str(int(v)))
def test_line_conv2d_forward_and_gradients(N, C, K, H, W, T, axis, bias, relu):
    x, w, b, pad = _case(N, C, K, H, W, T, axis, bias, 100 * T + 10 * C + H + axis)
    dy, ref, grads, ta, gterms = _reference(x, w, b, pad, relu)
    runs = []
    for _ in range(2):
        xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        bg = b.to(DEV).requires_grad_(True) if bias else None
        y = ops.line_conv2d(xg, wg, bg, relu=relu)
        y.backward(dy.to(DEV))
        runs.append((y.detach(), xg.grad, wg.grad) + ((bg.grad,) if bias else ()))
    assert all(torch.equal(a, c) for a, c in zip(*runs)), 'two calls on the same inputs differ'
    y, dx, dw = runs[0][:3]
    bounded('forward', y, ref, ta, T * C + 2)
    bounded('dgrad', dx, grads[0], gterms[0], T * K + 1)
    bounded('wgrad', dw, grads[1], gterms[1], N * H * W + 1)
    if bias:
        bounded('bias grad', runs[0][3], grads[2], gterms[2], N * H * W + 1)


def test_c_entries_slabs_workspace_and_domain():
    N, C, K, H, W, T = 3, 20, 36, 17, 19, 7
    numel = K * T * C
    wsb = int(lib.nnl_lineconv2d_wgrad_workspace_bytes(N, H, W, C, K, T, AX_W))
    assert wsb >= 2 * numel * 4 and wsb % (numel * 4) == 0, 'workspace %d B: fewer than two slabs' % wsb
    assert int(lib.nnl_lineconv2d_wgrad_workspace_bytes(1, 2, 3, C, K, T, AX_W)) == 0, 'a 6-pixel problem is one slab'
    x, w, _, pad = _case(N, C, K, H, W, T, AX_W, False, 11)
    dy, _, grads, _, gterms = _reference(x, w, None, pad, False)
    xn, dyn = (t.permute(0, 2, 3, 1).contiguous().to(DEV) for t in (x, dy))
    outs = []
    for _ in range(2):
        dw, ws = torch.empty(K, T, C, device=DEV), torch.empty(wsb // 4, device=DEV)
        assert lib.nnl_lineconv2d_wgrad(ptr(xn), ptr(dyn), ptr(dw), ptr(ws), wsb, N, H, W, C, K, T, AX_W, None) == 0
        outs.append(dw)
    assert torch.equal(*outs)
    bounded('wgrad, %d slabs' % (wsb // (numel * 4)), outs[0], grads[1].permute(0, 3, 2, 1).reshape(K, T, C), gterms[1].permute(0, 3, 2, 1).reshape(K, T, C),
            N * H * W + 1)
    sentinel = torch.full((K, T, C), 7.0, device=DEV)
    assert lib.nnl_lineconv2d_wgrad(ptr(xn), ptr(dyn), ptr(sentinel), ptr(ws), wsb - 4, N, H, W, C, K, T, AX_W, None) != 0, 'short workspace accepted'
    wn, y = w.permute(0, 2, 3, 1).contiguous().to(DEV), torch.full((N, H, W, K), 7.0, device=DEV)

    def fwd(px=xn, pw=wn, py=y, C=C, T=T, axis=AX_W):
        return lib.nnl_lineconv2d_fwd(ptr(px), ptr(pw), None, ptr(py), N, H, W, C, K, T, axis, 0, 0, None)
    for what, kw in {'T = 4': dict(T=4), 'T = 9': dict(T=9), 'axis 2': dict(axis=2), 'C = 6': dict(C=6), 'null x': dict(px=None),
                     'null w': dict(pw=None), 'null y': dict(py=None)}.items():
        assert fwd(**kw) != 0, what
        if not what.startswith('null'):
            args = (N, H, W, kw.get('C', C), K, kw.get('T', T), kw.get('axis', AX_W))
            assert int(lib.nnl_lineconv2d_wgrad_workspace_bytes(*args)) == 0, what
            assert lib.nnl_lineconv2d_wgrad(ptr(xn), ptr(dyn), ptr(sentinel), ptr(ws), wsb, *args, None) != 0, what
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((sentinel == 7.0).all()), 'a refused call wrote its output'
