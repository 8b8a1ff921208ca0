"""K21 bf16 matrix-core convolutions (csrc/conv_bf16.hip) through ops.conv2d_bf16 and the C entries, against the same composition in fp64 on
operands rounded exactly as the kernels round them, rb(t) = t.bfloat16().double(): forward act(F.conv2d(rb(x), rb(w), b)), dx from
rb(dy gate) and rb(w), dw from rb(x) and rb(dy gate), db from the unrounded gated dy.

A bf16 x bf16 product is exact in fp32, so what remains is fp32 accumulation: bound and `bounded` helper of tests/test_dwconv_gpu.py, per
value n 2^-24 sum|terms| with the sum from the same composition on absolute rounded operands; n = R S C + 3 forward, R S K + 2 for dx,
N P Q + 2 for dw and db.  Every case runs twice: torch.equal.
Seed conditions (asserted, checkable on the CPU): no fp64 pre-activation of a ReLU case lies within the forward bound of zero, so the fp32
and the fp64 gate agree; and in a sigmoid case, where the fp32 gate y (1 - y) follows the fp64 one to the relative size d of the forward
bound (|d ln gate / d pre| <= 1) plus 8 x 2^-24 of its own arithmetic, no gated dy lies within d of a bf16 rounding boundary, so both round
to the same bf16."""
import pytest
import torch
import torch.nn.functional as F

from test_dwconv_gpu import U, bounded

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (R, stride, pad, C, K, (N, H, W), bias, act, slot, seed) — what each shape is for, with 64-pixel x 64-channel tiles, k-steps of 4 chunks of 8
# channels (forward / dgrad) and 64-pixel steps in slabs of at least 256 pixels (wgrad).  slot: 'take' passes a GradSlot holding a shortcut,
# 'give' an open give_slot
CASES = [
    (1, 1, 0, 8, 8, (1, 3, 5), False, 0, None, 1),          # 15 pixels, one chunk: one partial tile of everything, three zero chunks in the only k-step
    (3, 1, 1, 24, 40, (2, 7, 9), False, 1, None, 2),        # 27 chunks = 6 k-steps + 3: a k-step tail, steps that straddle taps, a column-tile tail, all four borders
    (3, 2, 1, 16, 24, (2, 9, 11), False, 1, None, 3),       # odd sizes at stride 2: the dgrad's stride predicate, dx rows and columns of both parities
    (1, 2, 0, 32, 72, (3, 8, 8), False, 0, None, 4),        # the projection shortcut: 3 of 4 dx pixels receive nothing; K one tile + 8
    (5, 1, 2, 48, 64, (1, 6, 6), False, 1, None, 21),       # 25 taps, a pad of 2, 6 chunks per tap against 4 per step
    (3, 1, 0, 8, 8, (1, 5, 5), True, 2, None, 17),          # no padding, bias and the sigmoid epilogue / gate
    (3, 1, 1, 64, 64, (4, 17, 19), True, 0, None, 7),       # 1292 pixels: 21 row tiles, 6 wgrad slabs (the last one short), the bias gradient; no
                                                            # ReLU: among 82688 pre-activations some always lie within the bound of zero
    (1, 1, 0, 8, 264, (1, 4, 4), False, 0, None, 8),        # K = 4 column tiles + 8: the forward's column walk, the dgrad's 33-chunk reduction
    (3, 1, 1, 16, 16, (2, 6, 6), False, 1, 'take', 9),      # the GradSlot shortcut: added in the dgrad epilogue, exactly once
    (1, 2, 0, 16, 32, (2, 6, 6), False, 0, 'give', 10),     # an open give_slot: dx is parked, autograd gets None
]


def rb(t):
    return t.bfloat16().double()


def _case(R, C, K, nhw, bias, seed):
    g = torch.Generator().manual_seed(seed)
    N, H, W = nhw
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / (R * R * C) ** 0.5
    b = torch.randn(K, generator=g) if bias else None
    return x, w, b, g


def _reference(x, w, b, stride, pad, act, g):
    "fp64 output, [dx, dw, (db)], the sums of absolute terms of each, and dy (drawn here: its shape is the output's)"
    R, C = w.shape[2], w.shape[1]
    leaf = lambda t: t.clone().requires_grad_(True)                                                                           # noqa: E731
    b64 = None if b is None else b.double()
    xr, wr = leaf(rb(x)), leaf(rb(w))
    pre = F.conv2d(xr, wr, b64, stride, pad)
    ta = F.conv2d(rb(x).abs(), rb(w).abs(), None if b is None else b64.abs(), stride, pad)
    dy = torch.randn(pre.shape, generator=g)
    sg = torch.sigmoid(pre.detach())
    gate = [torch.ones_like(sg), (pre.detach() > 0).double(), sg * (1 - sg)][act]
    gd = dy.double() * gate                                           # the gated output gradient; the kernels see it rounded to bf16
    n_f = R * R * C + 3
    if act == 1:
        near = pre.detach().abs() <= n_f * U * ta
        assert not bool(near.any()), 'seed condition: %d pre-activations lie within the forward bound of zero' % int(near.sum())
    if act == 2:
        d = n_f * U * ta + 8 * U
        flips = rb((gd - gd.abs() * d).float()) != rb((gd + gd.abs() * d).float())
        assert not bool(flips.any()), 'seed condition: %d gated gradients lie within the gate error of a bf16 rounding boundary' % int(flips.sum())
    ref = [pre, torch.relu(pre), torch.sigmoid(pre)][act].detach()
    gdr = rb(gd.float())
    dx, dw = torch.autograd.grad(F.conv2d(xr, wr, None, stride, pad), (xr, wr), gdr)
    xa, wa = leaf(rb(x).abs()), leaf(rb(w).abs())
    dxa, dwa = torch.autograd.grad(F.conv2d(xa, wa, None, stride, pad), (xa, wa), gdr.abs())
    grads, terms = [dx, dw], [dxa, dwa]
    if b is not None:
        grads.append(gd.sum((0, 2, 3)))
        terms.append(gd.abs().sum((0, 2, 3)))
    return ref, grads, [ta] + terms, dy


@pytest.mark.parametrize('R,stride,pad,C,K,nhw,bias,act,slot,seed', CASES, ids=[str(i + 1) for i in range(len(CASES))])
def test_conv2d_bf16_forward_and_gradients(R, stride, pad, C, K, nhw, bias, act, slot, seed):
    x, w, b, g = _case(R, C, K, nhw, bias, seed)
    ref, grads, terms, dy = _reference(x, w, b, stride, pad, act, g)
    shortcut = torch.randn(nhw[0], nhw[1], nhw[2], C, generator=g)            # NHWC, as the closing BatchNorm parks it
    runs = []
    for _ in range(2):
        leaves = [t.to(DEV).requires_grad_(True) for t in [x, w.contiguous(memory_format=torch.channels_last)] + ([b] if bias else [])]
        take, give = ops.GradSlot(), ops.GradSlot()
        take.tensor = shortcut.to(DEV)
        y = ops.conv2d_bf16(leaves[0], leaves[1], leaves[2] if bias else None, stride, pad, relu=act, grad_slot=take if slot == 'take' else None,
                            give_slot=give if slot == 'give' else None)
        y.backward(dy.to(DEV))
        if slot == 'take':
            assert take.closed and take.tensor is None, 'the consumer must take the shortcut and close the slot'
        if slot == 'give':
            assert leaves[0].grad is None and give.tensor is not None, 'dx must be parked in the open slot, not returned to autograd'
            leaves[0].grad = give.tensor.permute(0, 3, 1, 2)
        runs.append([y.detach()] + [t.grad for t in leaves])
    assert all(torch.equal(a, c) for a, c in zip(*runs)), 'two calls on the same inputs differ'
    got, M = runs[0], ref.numel() // K
    if slot == 'take':                                                 # one more addition per value, of the shortcut
        grads[0], terms[1] = grads[0] + shortcut.permute(0, 3, 1, 2).double(), terms[1] + shortcut.permute(0, 3, 1, 2).abs().double()
    bounded('forward', got[0], ref, terms[0], R * R * C + 3)
    bounded('input grad', got[1], grads[0], terms[1], R * R * K + 2 + (slot == 'take'))
    bounded('weight grad', got[2], grads[1], terms[2], M + 2)
    assert got[2].stride() == leaves[1].stride(), 'the weight gradient is not in the parameter strides'
    if bias:
        bounded('bias grad', got[3], grads[2], terms[3], M + 2)


def test_conv2d_bf16_refuses_outside_its_domain():
    x = torch.zeros(1, 8, 4, 4)
    for what, args in {'kernel_size': (x, torch.zeros(8, 8, 1, 3), 1, 0), 'stride': (x, torch.zeros(8, 8, 1, 1), 3, 0),
                       'in_channels': (torch.zeros(1, 12, 4, 4), torch.zeros(8, 12, 1, 1), 1, 0), 'out_channels': (x, torch.zeros(12, 8, 1, 1), 1, 0),
                       'padding': (x, torch.zeros(8, 8, 7, 7), 1, 1)}.items():
        with pytest.raises(NotImplementedError, match=what):
            ops.conv2d_bf16(args[0], args[1], None, args[2], args[3])


def test_c_entries_slabs_workspace_and_domain():
    R, stride, pad, C, K, nhw = 3, 1, 1, 16, 24, (3, 17, 19)
    geom = lambda **kw: ops._geom(*[kw.get(k, v) for k, v in zip('NHWCKRS', nhw + (C, K, R, R))], kw.get('stride', stride), kw.get('pad', pad))     # noqa: E731
    g0, M, numel = geom(), 3 * 17 * 19, K * R * R * C
    wsb = int(lib.nnl_conv2d_bf16_wgrad_workspace_bytes(g0))
    assert wsb >= 2 * numel * 4 and wsb % (numel * 4) == 0, 'workspace %d B: fewer than two slabs' % wsb
    assert int(lib.nnl_conv2d_bf16_wgrad_workspace_bytes(geom(N=1, H=3, W=2))) == 0, 'a 6-pixel problem is one slab'
    x, w, _, g = _case(R, C, K, nhw, False, 11)
    _, grads, terms, dy = _reference(x, w, None, stride, pad, 0, g)
    xn, dyn = (t.permute(0, 2, 3, 1).contiguous().to(DEV) for t in (x, dy))
    outs = []
    for _ in range(2):
        dw, ws = torch.empty(K, R, R, C, device=DEV), torch.empty(wsb // 4, device=DEV)
        assert lib.nnl_conv2d_bf16_wgrad(ptr(xn), ptr(dyn), ptr(dw), g0, ptr(ws), wsb, None) == 0
        outs.append(dw)
    assert torch.equal(*outs)
    bounded('wgrad, %d slabs' % (wsb // (numel * 4)), outs[0].permute(0, 3, 1, 2), grads[1], terms[2], M + 2)
    sentinel = torch.full((K, R, R, C), 7.0, device=DEV)
    assert lib.nnl_conv2d_bf16_wgrad(ptr(xn), ptr(dyn), ptr(sentinel), g0, ptr(ws), wsb - 4, None) != 0, 'short workspace accepted'
    y, wp = torch.full((M, K), 7.0, device=DEV), torch.zeros(numel, dtype=torch.bfloat16, device=DEV)
    dx = torch.full((M, C), 7.0, device=DEV)
    for what, kw in {'C = 12': dict(C=12), 'K = 12': dict(K=12), 'stride 3': dict(stride=3), 'R S > 49': dict(R=8, S=8, pad=4), 'null pointer': {}}.items():
        gb, null = geom(**kw), what == 'null pointer'
        assert lib.nnl_conv2d_bf16_supported(gb) == null, what
        assert lib.nnl_conv2d_bf16_fwd(None if null else ptr(xn), ptr(wp), None, ptr(y), gb, 0, None) != 0, what
        assert lib.nnl_conv2d_bf16_dgrad(None if null else ptr(dyn), ptr(wp), ptr(dx), gb, None, None) != 0, what
        assert lib.nnl_conv2d_bf16_wgrad(None if null else ptr(xn), ptr(dyn), ptr(sentinel), gb, ptr(ws), wsb, None) != 0, what
        assert null or int(lib.nnl_conv2d_bf16_wgrad_workspace_bytes(gb)) == 0, what
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (y, dx, sentinel)), 'a refused call wrote its output'
