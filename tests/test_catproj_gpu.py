"""K20 concat-fused residual projection (csrc/catproj.hip) through ops.cat_conv1x1_residual and the C entries, against the same composition
in fp64: torch.cat -> F.conv2d (1 x 1) -> * scale -> + residual -> relu, and its autograd.

Bound and `bounded` helper of tests/test_dwconv_gpu.py: per value n 2^-24 sum|terms|, the sum from the same fp64 composition on absolute
operands; it holds for any summation order, so neither the forward's filter-range split nor the wgrad slabs change it.  n = Ctot + 4 forward
(Ctot products and additions, bias, scale, residual, one spare), K + 2 source gradients, M + 2 weight and bias gradients; the residual's
gradient is dy where the gate is open and 0 elsewhere, exactly.  Every case runs twice: torch.equal.
The seeds are chosen so that no fp64 pre-activation of a ReLU case lies within the forward bound of zero (asserted): the fp32 gate and the
fp64 gate then agree on every element."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_dwconv_gpu import U, bounded

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (sources, K, (N, H, W), bias, relu, residual, scale, seed) — what each shape is for, with 64-row / 64-filter / 64-column tiles and 16-channel chunks:
CASES = [
    ((4,), 4, (1, 3, 5), False, False, False, 1.0, 1),             # M = 15: one partial tile of everything
    ((4, 20, 44), 36, (3, 5, 17), True, True, True, 0.17, 2),      # M = 255: a dgrad column tile over two source boundaries, a 4-column tail tile,
                                                                   # a chunk tail (68 = 4 x 16 + 4), a filter-tile tail, a last row tile of 63
    ((32, 32, 64), 320, (1, 9, 9), True, True, True, 0.17, 13),    # Block35's own split
    ((192, 192), 68, (2, 8, 8), True, True, True, 0.10, 4),        # a panel above 64 KB
    ((256, 256), 4, (1, 7, 10), True, True, True, 0.10, 15),       # the largest legal panel
    ((192, 256), 2080, (1, 8, 8), True, False, True, 1.0, 6),      # Block8 at one image: 33 filter tiles shared out by the planner
    ((4, 4, 4, 4), 8, (3, 17, 19), True, True, True, 0.20, 7),     # M = 969: four sources
]


def _case(sources, K, nhw, bias, residual, seed):
    g = torch.Generator().manual_seed(seed)
    N, H, W = nhw
    xs = [torch.randn(N, c, H, W, generator=g) for c in sources]
    w = torch.randn(K, sum(sources), 1, 1, generator=g) / sum(sources) ** 0.5
    b = torch.randn(K, generator=g) if bias else None
    r = torch.randn(N, K, H, W, generator=g) if residual else None
    return xs, w, b, r, torch.randn(N, K, H, W, generator=g)


def _compose(xs, w, b, r, scale):
    pre = F.conv2d(torch.cat(xs, 1), w, b) * scale
    return pre if r is None else pre + r


def _reference(xs, w, b, r, dy, scale, relu):
    "fp64 output and gradients (sources, weight, bias), the sums of absolute terms of each, and the gate"
    leaves = lambda f: ([f(x).double().requires_grad_(True) for x in xs], f(w).double().requires_grad_(True),                  # noqa: E731
                        None if b is None else f(b).double().requires_grad_(True), None if r is None else f(r).double())
    xr, wr, br, rr = leaves(lambda t: t)
    pre = _compose(xr, wr, br, rr, scale)
    ref = torch.relu(pre) if relu else pre
    ref.backward(dy.double())
    xa, wa, ba, ra = leaves(torch.abs)
    ta = _compose(xa, wa, ba, ra, scale)
    gate = (pre > 0).double() if relu else torch.ones_like(pre)
    ta.backward(dy.abs().double() * gate)
    grads = lambda xl, wl, bl: [x.grad for x in xl] + [wl.grad] + ([] if bl is None else [bl.grad])                           # noqa: E731
    if relu:
        near = pre.detach().abs() <= (sum(x.shape[1] for x in xs) + 4) * U * ta.detach()
        assert not bool(near.any()), 'seed condition: %d pre-activations lie within the forward bound of zero' % int(near.sum())
    return ref.detach(), grads(xr, wr, br), ta.detach(), grads(xa, wa, ba), gate


@pytest.mark.parametrize('sources,K,nhw,bias,relu,residual,scale,seed', CASES, ids=[str(i + 1) for i in range(len(CASES))])
def test_cat_conv1x1_residual_forward_and_gradients(sources, K, nhw, bias, relu, residual, scale, seed):
    xs, w, b, r, dy = _case(sources, K, nhw, bias, residual, seed)
    ref, grads, ta, gterms, gate = _reference(xs, w, b, r, dy, scale, relu)
    M, Ctot = nhw[0] * nhw[1] * nhw[2], sum(sources)
    runs = []
    for _ in range(2):
        leaves = [t.to(DEV).requires_grad_(True) for t in xs + [w] + ([b] if bias else []) + ([r] if residual else [])]
        xg, wg = leaves[:len(xs)], leaves[len(xs)]
        y = ops.cat_conv1x1_residual(xg, wg, leaves[len(xs) + 1] if bias else None, leaves[-1] if residual else None, scale, relu=relu)
        y.backward(dy.to(DEV))
        runs.append([y.detach()] + [t.grad for t in leaves])
    assert all(torch.equal(a, c) for a, c in zip(*runs)), 'two calls on the same inputs differ'
    got = runs[0]
    bounded('forward', got[0], ref, ta, Ctot + 4)
    names = ['source %d grad' % s for s in range(len(xs))] + ['weight grad'] + ['bias grad'] * bias
    for name, have, want, terms in zip(names, got[1:], grads, gterms):
        bounded(name, have, want, terms, K + 2 if name.startswith('source') else M + 2)
    if residual:
        assert torch.equal(got[-1].cpu(), dy * gate.float()), 'the residual gradient is not dy under the gate, exactly'


def test_c_entries_slabs_workspace_and_domain():
    sources, K, nhw = (4, 20, 44), 36, (3, 17, 19)
    M, Ctot = 3 * 17 * 19, 68
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)                                                                           # noqa: E731
    ptrs = lambda *t: (ctypes.c_void_p * len(t))(*[None if a is None else a.data_ptr() for a in t])                           # noqa: E731
    ch = i64s(*sources)
    wsb = int(lib.nnl_catproj_wgrad_workspace_bytes(ch, 3, M, K))
    assert wsb >= 2 * K * Ctot * 4 and wsb % (K * Ctot * 4) == 0, 'workspace %d B: fewer than two slabs' % wsb
    assert int(lib.nnl_catproj_wgrad_workspace_bytes(ch, 3, 6, K)) == 0, 'a 6-row problem is one slab'
    xs, w, _, _, dy = _case(sources, K, nhw, False, False, 11)
    _, grads, _, gterms, _ = _reference(xs, w, None, None, dy, 0.5, False)
    xn = [x.permute(0, 2, 3, 1).contiguous().to(DEV) for x in xs]
    dyn, wn = dy.permute(0, 2, 3, 1).contiguous().to(DEV), w.reshape(K, Ctot).to(DEV)
    outs = []
    for _ in range(2):
        dw, ws = torch.empty(K, Ctot, device=DEV), torch.empty(wsb // 4, device=DEV)
        assert lib.nnl_catproj_wgrad(ptrs(*xn), ch, 3, ptr(dyn), None, ptr(dw), ptr(ws), wsb, M, K, 0.5, 0, None) == 0
        outs.append(dw)
    assert torch.equal(*outs)
    bounded('wgrad, %d slabs' % (wsb // (K * Ctot * 4)), outs[0], grads[3].reshape(K, Ctot), gterms[3].reshape(K, Ctot), M + 2)
    sentinel = torch.full((K, Ctot), 7.0, device=DEV)
    assert lib.nnl_catproj_wgrad(ptrs(*xn), ch, 3, ptr(dyn), None, ptr(sentinel), ptr(ws), wsb - 4, M, K, 0.5, 0, None) != 0, 'short workspace accepted'
    y = torch.full((M, K), 7.0, device=DEV)
    five = xn + xn[:2]

    def fwd(src=xn, chans=sources, n=3, pw=wn, py=y, K=K):
        return lib.nnl_catproj_fwd(ptrs(*src), i64s(*chans), n, ptr(pw), None, None, ptr(py), M, K, 1.0, 0, None)
    for what, kw in {'C_s = 6': dict(chans=(6, 20, 44)), 'Ctot = 516': dict(chans=(4, 20, 492)), 'n_src = 0': dict(n=0),
                     'n_src = 5': dict(src=five, chans=(4, 20, 44, 4, 20), n=5), 'K = 6': dict(K=6), 'null source': dict(src=[xn[0], None, xn[2]]),
                     'null w': dict(pw=None), 'null y': dict(py=None)}.items():
        assert fwd(**kw) != 0, what
        if not what.startswith('null'):
            args = (i64s(*kw.get('chans', sources)), kw.get('n', 3))
            assert int(lib.nnl_catproj_wgrad_workspace_bytes(*args, M, kw.get('K', K))) == 0, what
            assert lib.nnl_catproj_wgrad(ptrs(*kw.get('src', xn)), *args, ptr(dyn), None, ptr(sentinel), ptr(ws), wsb, M, kw.get('K', K), 0.5, 0, None) != 0, what
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((sentinel == 7.0).all()), 'a refused call wrote its output'
