"""K22 bf16 matrix-core Linear (csrc/linear_bf16.hip) through ops.linear_bf16 and the C entries, against the same composition in fp64 on
operands rounded exactly as the kernels round them, rb(t) = t.bfloat16().double(): y = act(rb(x) rb(w)^T + b), dx = rb(dy gate) rb(w),
dw = rb(dy gate)^T rb(x), db = the column sums of the unrounded gated dy.

A bf16 x bf16 product is exact in fp32, so what remains is fp32 accumulation: bound and `bounded` helper of tests/test_dwconv_gpu.py, per
value n 2^-24 sum|terms| with the sum from the same composition on absolute rounded operands; n = K + 3 forward, N + slabs + 2 for dx,
M + slabs + 2 for dw and db, the slab counts read from the workspace entries.  Every case runs twice: torch.equal.
Seed condition (asserted, checkable on the CPU): no fp64 pre-activation of a ReLU case lies within the forward bound of zero, so the fp32
and the fp64 gate agree."""
import pytest
import torch

from test_dwconv_gpu import U, bounded
from test_gconv_mfma_gpu import routes

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (M, N, K, bias, relu, ldx, lddy, seed) — what each shape is for, with 128 x 128 output tiles, reduction steps of 32 (4 chunks of 8) and
# backward slabs of at least 512.  ldx / lddy 0: dense; lddy > 0: dy is a view over a base registered with register_padded_grad
CASES = [
    (3, 5, 7, False, False, 0, 0, 1),          # one partial tile of everything; rows of 7 and 5 floats: the dword path of every operand
    (40, 9, 46, False, False, 0, 0, 2),        # K = 8 x 5 + 6: not a multiple of the MFMA k-step of 16: a half-empty chunk and an empty one
    (70, 20, 100, True, False, 0, 0, 3),       # K = 3 W steps + 4: a chunk tail inside the last step; the bias epilogue
    (6, 133, 24, False, False, 0, 144, 4),     # N = one column tile + 1 in a padded base of 144: the _SoftmaxCE hand-over, read in place
    (300, 140, 40, False, False, 0, 0, 5),     # three row tiles, the last one of 44 rows; two column tiles, the second 12 wide
    (40, 1300, 24, False, False, 0, 0, 6),     # dgrad: three N slabs of 512, 512, 276, folded in slab order
    (1300, 24, 40, True, False, 0, 0, 7),      # wgrad: three M slabs of 512, 512, 276, the bias partials folded with them
    (37, 50, 33, True, True, 0, 0, 8),         # bias + ReLU with a bias gradient from the gated dy
    (20, 30, 16, False, False, 20, 0, 9),      # a row-strided x (ldx 20 > K 16), read in place by the forward and the wgrad
    (5, 130, 2300, False, False, 0, 0, 10),    # a 72-step forward reduction over two column tiles; one dgrad step per row of W
    (5, 70000, 8, False, False, 0, 0, 11),     # 547 column tiles of one row tile; a dgrad of 16 slabs, the most the planner makes,
                                               # the last one short
]


def rb(t):
    return t.bfloat16().double()


def _reference(M, N, K, bias, relu, seed):
    "inputs, the fp64 output and [dx, dw, (db)], and the sums of absolute terms of each"
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    dy = torch.randn(M, N, generator=g)
    pre = rb(x) @ rb(w).T + (b.double() if bias else 0)
    ta = rb(x).abs() @ rb(w).abs().T + (b.double().abs() if bias else 0)
    if relu:
        near = pre.abs() <= (K + 3) * U * ta
        assert not bool(near.any()), 'seed condition: %d pre-activations lie within the forward bound of zero' % int(near.sum())
    gd = dy.double() * (pre > 0) if relu else dy.double()              # the gated output gradient; the kernels see it rounded to bf16
    gdr = rb(gd.float())
    grads, terms = [gdr @ rb(w), gdr.T @ rb(x)], [ta, gdr.abs() @ rb(w).abs(), gdr.abs().T @ rb(x).abs()]
    if bias:
        grads.append(gd.sum(0))
        terms.append(gd.abs().sum(0))
    return (x, w, b, dy), torch.relu(pre) if relu else pre, grads, terms


def _slabs(M, N, K):
    "(dgrad, wgrad) slab counts, from the workspace entries"
    d, w = int(lib.nnl_linear_bf16_dgrad_workspace_bytes(M, N, K)), int(lib.nnl_linear_bf16_wgrad_workspace_bytes(M, N, K))
    assert d % (M * K * 4) == 0 and w % ((N * K + N) * 4) == 0
    return max(1, d // (M * K * 4)), max(1, w // ((N * K + N) * 4))


@pytest.mark.parametrize('M,N,K,bias,relu,ldx,lddy,seed', CASES, ids=[str(i + 1) for i in range(len(CASES))])
def test_linear_bf16_forward_and_gradients(M, N, K, bias, relu, ldx, lddy, seed):
    (x, w, b, dy), ref, grads, terms = _reference(M, N, K, bias, relu, seed)
    sd, sw = _slabs(M, N, K)
    assert sd >= 3 or (M, N, K) != (40, 1300, 24), 'the dgrad case no longer has three slabs'
    assert sw >= 3 or (M, N, K) != (1300, 24, 40), 'the wgrad case no longer has three slabs'
    runs = []
    for _ in range(2):
        xd = torch.nn.functional.pad(x, (0, ldx - K)).to(DEV)[:, :K] if ldx else x.to(DEV)
        leaves = [t.requires_grad_(True) for t in [xd.detach(), w.to(DEV)] + ([b.to(DEV)] if bias else [])]
        dyd = dy.to(DEV)
        if lddy:
            base = torch.nn.functional.pad(dy, (0, lddy - N)).to(DEV)
            ops.register_padded_grad(base, lddy)
            dyd = base[:, :N]
            used, ld = ops._linear_bf16_dy(dyd, N)
            assert used.data_ptr() == base.data_ptr() and ld == lddy and tuple(used.shape) == (M, lddy), 'the padded base is not used as is'
        y = ops.linear_bf16(leaves[0], leaves[1], leaves[2] if bias else None, relu=relu)
        _, notes = routes(lambda: y.backward(dyd))
        assert not lddy or not any(':dword' in n for n in notes), 'dy left its 16-byte aligned padded rows: %s' % notes
        runs.append([y.detach()] + [t.grad for t in leaves])
    assert all(torch.equal(a, c) for a, c in zip(*runs)), 'two calls on the same inputs differ'
    got = runs[0]
    bounded('forward', got[0], ref, terms[0], K + 3)
    bounded('input grad, %d slabs' % sd, got[1], grads[0], terms[1], N + sd + 2)
    bounded('weight grad, %d slabs' % sw, got[2], grads[1], terms[2], M + sw + 2)
    assert got[2].stride() == leaves[1].stride(), 'the weight gradient is not in the parameter strides'
    if bias:
        bounded('bias grad', got[3], grads[2], terms[3], M + sw + 2)


def test_c_entries_workspace_and_domain():
    M, N, K = 1300, 24, 40
    assert _slabs(3, 5, 7) == (1, 1) and int(lib.nnl_linear_bf16_dgrad_workspace_bytes(3, 5, 7)) == 0 \
        and int(lib.nnl_linear_bf16_wgrad_workspace_bytes(3, 5, 7)) == 0, 'a one-slab problem needs no workspace'
    wsb, dsb = int(lib.nnl_linear_bf16_wgrad_workspace_bytes(M, N, K)), int(lib.nnl_linear_bf16_dgrad_workspace_bytes(N, M, K))
    assert wsb > 0 and dsb > 0
    x, dy, w = torch.randn(M, K, device=DEV), torch.randn(M, N, device=DEV), torch.randn(N, K, device=DEV)
    ws = torch.empty(max(wsb, dsb) // 4, device=DEV)
    y, dx, dw, db = (torch.full(s, 7.0, device=DEV) for s in ((M, N), (M, K), (N, K), (N,)))
    dxs = torch.full((N, K), 7.0, device=DEV)                          # the sliced dgrad: N rows, a reduction over M
    fwd = lambda **k: lib.nnl_linear_bf16_fwd(k.get('x', ptr(x)), ptr(w), None, ptr(y), k.get('M', M), N, K, k.get('ldx', K), K, k.get('ldy', N), 0, None)      # noqa: E731
    dgr = lambda **k: lib.nnl_linear_bf16_dgrad(k.get('dy', ptr(dy)), ptr(w), ptr(dx), M, k.get('N', N), K, k.get('lddy', N), k.get('ldw', K), None, 0, None)   # noqa: E731
    wgr = lambda **k: lib.nnl_linear_bf16_wgrad(k.get('x', ptr(x)), ptr(dy), ptr(dw), ptr(db), M, N, K, k.get('ldx', K), k.get('lddy', N),       # noqa: E731
                                                k.get('ws', ptr(ws)), k.get('wsb', wsb), None)
    refused = {'null x': [fwd(x=None), wgr(x=None)], 'null dy': [dgr(dy=None)], 'short ldx': [fwd(ldx=K - 1), wgr(ldx=K - 1)], 'short ldy': [fwd(ldy=N - 1)],
               'short lddy': [dgr(lddy=N - 1), wgr(lddy=N - 1)], 'short ldw': [dgr(ldw=K - 1)], 'M = 0': [fwd(M=0)], 'N < 0': [dgr(N=-3)],
               'short workspace': [wgr(wsb=wsb - 4), lib.nnl_linear_bf16_dgrad(ptr(dy), ptr(x), ptr(dxs), N, M, K, M, K, ptr(ws), dsb - 4, None)],
               'null workspace': [wgr(ws=None)]}
    for what, codes in refused.items():
        assert all(c != 0 for c in codes), what + ' accepted'
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (y, dx, dw, db, dxs)), 'a refused call wrote its output'
