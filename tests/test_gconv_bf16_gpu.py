"""K24 bf16 matrix-core grouped convolutions (csrc/gconv_bf16.hip) through ops.grouped_conv2d_bf16 and the C entries, with the method of
tests/test_conv_bf16_gpu.py: the reference is the same composition in fp64 on operands rounded exactly as the kernels round them,
rb(t) = t.bfloat16().double(): forward relu?(F.conv2d(rb(x), rb(w), b, groups=G)), dx and dw from rb(gated dy), db from the unrounded gated dy.

A bf16 x bf16 product is exact in fp32, so what remains is fp32 accumulation: bound and `bounded` helper of tests/test_dwconv_gpu.py, per
value n 2^-24 sum|terms| with the sum from the same composition on absolute rounded operands; n = R R Cg + 3 forward, R R Kg + 2 for dx,
N P Q + 2 for dw and db.  Every case runs twice: torch.equal.
Seed condition (asserted, checkable on the CPU): no fp64 pre-activation of a ReLU case lies within the forward bound of zero, so the fp32
and the fp64 gate agree."""
import pytest
import torch
import torch.nn.functional as F

from test_dwconv_gpu import U, bounded

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib, ptr

DEV = 'cuda'

# (R, stride, pad, C, K, G, (N, H, W), bias, relu, seed) — what each shape is for, with spans of 32 reduction channels, tiles of 16 columns
# and 8 x 8 pixels (forward / dgrad), and 32-pixel k-steps in slabs of at least 256 pixels (wgrad)
CASES = [
    (3, 1, 1, 8, 8, 2, (1, 3, 5), False, False, 1),         # 4/4, 15 pixels, a quarter span: one partial tile of everything
    (3, 1, 1, 16, 16, 4, (2, 6, 6), False, True, 1),        # 4/4 with the ReLU gate into both gradients
    (3, 2, 1, 64, 64, 8, (2, 9, 11), True, True, 1),        # 8/8, two spans, stride 2 on odd sizes, bias and ReLU: dx rows and columns of both parities
    (3, 1, 1, 40, 80, 10, (1, 5, 5), False, False, 4),      # Cg 4 / Kg 8: a span tail of 32 + 8, five column tiles
    (3, 1, 1, 32, 64, 2, (1, 4, 4), False, False, 5),       # 16/32: a group's columns straddle two column tiles, the dgrad's reduction of 32 is a whole k
    (3, 1, 1, 96, 96, 3, (1, 7, 7), False, False, 6),       # 32/32: a dense span = one group, three spans, all four borders
    (3, 2, 1, 32, 32, 2, (3, 8, 8), False, False, 7),       # 16/16, stride 2 on even sizes: the last input row and column are reached by fewer taps
    (1, 1, 0, 32, 32, 8, (1, 4, 4), False, False, 8),       # the one-tap filter
    (3, 1, 1, 32, 32, 4, (4, 17, 19), True, False, 9),      # 1292 pixels: many pixel tiles, 6 wgrad slabs (the last one short), the bias gradient; no
                                                            # ReLU: among 41344 pre-activations some always lie within the bound of zero
    (3, 1, 0, 16, 16, 2, (1, 5, 5), False, False, 10),      # no padding
]


def rb(t):
    return t.bfloat16().double()


def _reference(R, stride, pad, C, K, G, nhw, bias, relu, seed):
    "the inputs, the fp64 output, [dx, dw, (db)], the sums of absolute terms of each, and dy"
    g = torch.Generator().manual_seed(seed)
    N, H, W = nhw
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C // G, R, R, generator=g) / (R * R * C // G) ** 0.5
    b = torch.randn(K, generator=g) if bias else None
    leaf = lambda t: t.clone().requires_grad_(True)                                                                           # noqa: E731
    b64 = None if b is None else b.double()
    xr, wr = leaf(rb(x)), leaf(rb(w))
    pre = F.conv2d(xr, wr, b64, stride, pad, 1, G)
    ta = F.conv2d(rb(x).abs(), rb(w).abs(), None if b is None else b64.abs(), stride, pad, 1, G)
    dy = torch.randn(pre.shape, generator=g)
    if relu:
        near = pre.detach().abs() <= (R * R * C // G + 3) * U * ta
        assert not bool(near.any()), 'seed condition: %d pre-activations lie within the forward bound of zero' % int(near.sum())
    gd = dy.double() * (pre.detach() > 0).double() if relu else dy.double()      # the gated output gradient; the kernels see it rounded to bf16
    gdr = rb(gd.float())
    dx, dw = torch.autograd.grad(F.conv2d(xr, wr, None, stride, pad, 1, G), (xr, wr), gdr)
    xa, wa = leaf(rb(x).abs()), leaf(rb(w).abs())
    dxa, dwa = torch.autograd.grad(F.conv2d(xa, wa, None, stride, pad, 1, G), (xa, wa), gdr.abs())
    grads, terms = [dx, dw], [ta, dxa, dwa]
    if bias:
        grads.append(gd.sum((0, 2, 3)))
        terms.append(gd.abs().sum((0, 2, 3)))
    return (x, w, b), (torch.relu(pre) if relu else pre).detach(), grads, terms, dy


@pytest.mark.gpu
@pytest.mark.parametrize('R,stride,pad,C,K,G,nhw,bias,relu,seed', CASES, ids=[str(i + 1) for i in range(len(CASES))])
def test_grouped_conv2d_bf16_forward_and_gradients(R, stride, pad, C, K, G, nhw, bias, relu, seed):
    (x, w, b), ref, grads, terms, dy = _reference(R, stride, pad, C, K, G, nhw, bias, relu, seed)
    runs = []
    for _ in range(2):
        leaves = [t.to(DEV).requires_grad_(True) for t in [x, w.contiguous(memory_format=torch.channels_last)] + ([b] if bias else [])]
        y = ops.grouped_conv2d_bf16(leaves[0], leaves[1], leaves[2] if bias else None, stride, pad, G, relu=relu)
        y.backward(dy.to(DEV))
        runs.append([y.detach()] + [t.grad for t in leaves])
    assert all(torch.equal(a, c) for a, c in zip(*runs)), 'two calls on the same inputs differ'
    got, M = runs[0], ref.numel() // K
    bounded('forward', got[0], ref, terms[0], R * R * C // G + 3)
    bounded('input grad', got[1], grads[0], terms[1], R * R * K // G + 2)
    bounded('weight grad', got[2], grads[1], terms[2], M + 2)
    assert got[2].stride() == leaves[1].stride(), 'the weight gradient is not in the parameter strides'
    if bias:
        bounded('bias grad', got[3], grads[2], terms[3], M + 2)


def test_grouped_conv2d_bf16_refuses_outside_its_domain():
    z = torch.zeros
    for what, x, w, stride, pad, G in [('channels per group 2', z(1, 4, 4, 4), z(8, 2, 3, 3), 1, 1, 2), ('channels per group 12', z(1, 24, 4, 4), z(8, 12, 3, 3), 1, 1, 2),
                                       ('kernel_size', z(1, 8, 6, 6), z(8, 4, 5, 5), 1, 1, 2), ('stride', z(1, 8, 6, 6), z(8, 4, 3, 3), 3, 1, 2),
                                       ('padding', z(1, 8, 6, 6), z(8, 4, 3, 3), 1, 2, 2), ('groups', z(1, 12, 4, 4), z(8, 4, 3, 3), 1, 1, 8)]:
        with pytest.raises(NotImplementedError, match=what):
            ops.grouped_conv2d_bf16(x, w, None, stride, pad, G)


@pytest.mark.gpu
def test_c_entries_slabs_workspace_and_domain():
    R, stride, pad, C, K, G, nhw = CASES[8][:7]
    dims = lambda **kw: tuple(kw.get(k, v) for k, v in zip(('N', 'H', 'W', 'C', 'K', 'G', 'R', 'stride', 'pad'), nhw + (C, K, G, R, stride, pad)))     # noqa: E731
    d0, M, numel = dims(), nhw[0] * nhw[1] * nhw[2], K * R * R * C // G
    wsb = int(lib.nnl_gconv2d_bf16_workspace_bytes(*d0))
    assert wsb >= 2 * numel * 4 and wsb % (numel * 4) == 0, 'workspace %d B: fewer than two slabs' % wsb
    c1 = CASES[0]
    assert int(lib.nnl_gconv2d_bf16_workspace_bytes(*c1[6], c1[3], c1[4], c1[5], c1[0], c1[1], c1[2])) == 0, 'a 15-pixel problem is one slab'
    xn, dyn, wn = torch.randn(M, C, device=DEV), torch.randn(M, K, device=DEV), torch.randn(numel, device=DEV)
    ws, full = torch.empty(wsb // 4, device=DEV), lambda n: torch.full((n,), 7.0, device=DEV)                                  # noqa: E731
    y, dx, dw = full(M * K), full(M * C), full(numel)
    assert lib.nnl_gconv2d_bf16_wgrad(ptr(xn), ptr(dyn), ptr(dw), ptr(ws), wsb - 4, *d0, None) != 0, 'short workspace accepted'
    for what, kw in {'Cg = 2': dict(G=16), 'Cg = 12': dict(C=48, K=48), 'R = 5': dict(R=5, pad=2), 'stride 3': dict(stride=3), 'pad 2': dict(pad=2),
                     'G does not divide C': dict(C=34), 'null pointer': {}}.items():
        db, null = dims(**kw), what == 'null pointer'
        assert lib.nnl_gconv2d_bf16_supported(*db) == null, what
        assert lib.nnl_gconv2d_bf16_fwd(None if null else ptr(xn), ptr(wn), None, ptr(y), *db, 0, None) != 0, what
        assert lib.nnl_gconv2d_bf16_dgrad(None if null else ptr(dyn), ptr(wn), ptr(dx), *db, None) != 0, what
        assert lib.nnl_gconv2d_bf16_wgrad(None if null else ptr(xn), ptr(dyn), ptr(dw), ptr(ws), wsb, *db, None) != 0, what
        assert null or int(lib.nnl_gconv2d_bf16_workspace_bytes(*db)) == 0, what
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (y, dx, dw)), 'a refused call wrote its output'
