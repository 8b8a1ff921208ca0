"""K23 fused bf16 decoder + softmax cross-entropy (csrc/linear_ce_bf16.hip) through ops.linear_cross_entropy_bf16 and the C entries, against
fp64 on operands rounded as the kernels round them, rb(t) = t.bfloat16().double(): z64 = rb(x) rb(w)^T, loss = lse(z64) - z64[target],
D64 = (softmax(z64) - onehot) g / M, dx64 = D64 rb(w), dw64 = D64^T rb(x).  U = 2^-24; every case runs twice: torch.equal.

Loss bound of row r.  B = (K + 3) U max_j sum_k |rb(x)||rb(w)| bounds the error of every fp32 logit of the row (the bound of
test_linear_bf16_gpu.py); lse is 1-Lipschitz in the largest logit error and z_t is a logit: 2 B.  The softmax arithmetic adds, with
R = max_j z - min_j z (every shift z - m' and every rescale m - m' lies in [-R, 0]), `ranges` read from the forward workspace entry and
T = column tiles - ranges + 1 (no range walks more tiles), relative to s along the longest path of one term:
  the shift z - m': R U;  expf: 2 U;  per tile the 15 adds of an accumulator, the add of the two accumulators and the add to the running
  sum, and exp + multiply of its rescale: 20 U T;  the rescale shifts m - m' of all tiles telescope: R U;  the 3 merges of the lanes that
  share a row and the ranges - 1 range merges, each shift + exp + multiply + add: (R + 4) U each;
so |d log s| <= (c + 1) U with c = 2 R + 2 + 20 T + (ranges + 2)(R + 4) (the + 1: second order);  logf: 2 U |log s|;  m + log s: U |lse|;
lse - z_t: U |loss|.  A row with a bad target has loss 0 exactly.  The mean: the mean of the row bounds + M U mean|loss|.

Gradient bound, per value.  p = exp(z - lse) in fp32 is off by p rel, rel = 2 B + the lse arithmetic above + U |z - lse| + 2 U (expf), plus
2^-126 where it underflows; subtracting the one-hot, g / M and the product round 3 times: dD = |g| / M (p rel + 2^-126) + 3 U |D64| + 2^-126,
elementwise and absolute, because at a target whose p is near 1 the RELATIVE error of p - 1 is unbounded.  The reference uses the unrounded D64
and allows the operand 2^-9 of it: sum (2^-9 |D64| + (1 + 2^-8) dD) |operand|.  One rounding to bf16 is off by up to 2^-8 of a value, which
a sum led by its target column shows (a single-operand kernel measured 0.75 - 1.53 of this bound), so the kernel carries D as TWO bf16
operands, hi = rb(D) and lo = rb(D - hi), off by 2^-16.  The fp32 accumulation adds n U sum (|D64| + dD) |operand|, n = N + slabs + 2 for dx
and M + slabs + 2 for dw, slabs read from the workspace entry."""
import math

import pytest
import torch

from test_dwconv_gpu import U, bounded

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (M, N, K, kind) with 128-column forward tiles in ranges of at least 2, 64 owned x 128 walked backward tiles, 32-deep steps, slabs >= 512
CASES = [
    (3, 5, 7, ''),             # one partial tile of everything; dword staging; targets in column 0 and column N - 1
    (6, 133, 24, ''),          # N = one column tile + 1: a tail tile one column wide with a target in it, 127 zero-filled columns beside it
    (300, 140, 40, ''),        # three forward row tiles, the last of 44 rows; five owned dx tiles; rows >= M must not reach dw
    (40, 1300, 24, ''),        # 6 vocabulary ranges of 2 tiles (the last of 1): the range merge; 3 dx slabs folded; 21 owned dw tiles
    (1300, 24, 40, ''),        # the dw kernel's walk over 11 row tiles in 3 slabs of M; 21 owned dx tiles
    (70, 300, 400, ''),        # the model's K: 4 accumulator chunks, the last 16 columns wide
    (5, 260, 509, ''),         # the top of the domain, rows not 16-byte aligned: dword staging of 16 steps, every accumulator chunk
    (40, 400, 24, 'large'),    # |z| up to about 60: the online rescale, row maxima forced into the first, a middle and the last column tile
    (8, 133, 24, 'bad'),       # target[2] = -1, target[5] = N: loss 0, no one-hot, the index-error flag
]


def rb(t):
    return t.bfloat16().double()


def _reference(M, N, K, kind, gout):
    g = torch.Generator().manual_seed(M + N + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    if kind == 'large':
        w *= 4
        for r, c in ((0, 5), (1, 200), (2, 399)):
            w[c] = 12 * x[r] / x[r].norm()
    x64, w64 = rb(x), rb(w)
    z = x64 @ w64.T
    if kind == 'large':
        assert (z.argmax(1)[:3] // 128).tolist() == [0, 1, 3] and float(z.abs().max()) > 50
    draw = torch.randint(0, N, (M,), generator=g)
    rows = torch.arange(M)
    target = torch.stack([torch.zeros(M, dtype=torch.long), torch.full((M,), N - 1), z.argmax(1), draw])[rows % 4, rows]
    if kind == 'bad':
        target[2], target[5] = -1, N
    ok = (target >= 0) & (target < N)
    tc = torch.where(ok, target, 0)
    lse = torch.logsumexp(z, 1)
    loss = torch.where(ok, lse - z[rows, tc], 0.0)
    onehot = torch.zeros(M, N, dtype=torch.double)
    onehot[rows[ok], target[ok]] = 1.0
    p = torch.exp(z - lse[:, None])
    D = (p - onehot) * gout / M
    ranges = int(lib.nnl_linear_ce_bf16_fwd_workspace_bytes(M, N, K)) // (3 * M * 4)
    tiles = math.ceil(N / 128)
    assert 1 <= ranges <= tiles
    B = (K + 3) * U * (x64.abs() @ w64.abs().T).max(1).values
    R = z.max(1).values - z.min(1).values
    c = 2 * R + 2 + 20 * (tiles - ranges + 1) + (ranges + 2) * (R + 4)
    lse_arith = U * (c + 1 + 2 * (lse - z.max(1).values).abs() + lse.abs())
    loss_bound = torch.where(ok, 2 * B + lse_arith + U * loss.abs(), 0.0)
    rel = (2 * B + lse_arith)[:, None] + U * (z - lse[:, None]).abs() + 2 * U
    dD = abs(gout) / M * (p * rel + 2.0 ** -126) + 3 * U * D.abs() + 2.0 ** -126
    return dict(x=x, w=w, target=target, ok=ok, loss=loss, loss_bound=loss_bound, D=D, dD=dD, dx=D @ w64, dw=D.T @ x64, x64=x64, w64=w64, ranges=ranges)


def _grad_bounded(what, got, ref, r, op, n):
    "the two derived terms of the module docstring, handed to `bounded` as the sum of terms that n U multiplies"
    D, dD = (r['D'], r['dD']) if what == 'dx' else (r['D'].T, r['dD'].T)
    allowed = (2.0 ** -9 * D.abs() + (1 + 2.0 ** -8) * dD) @ op.abs() + n * U * ((D.abs() + dD) @ op.abs())
    bounded(what, got, ref, allowed / (n * U), n)


@pytest.mark.parametrize('M,N,K,kind', CASES, ids=['%dx%dx%d%s' % c for c in CASES])
def test_linear_cross_entropy_bf16_against_fp64(M, N, K, kind):
    gout = 1.7
    r = _reference(M, N, K, kind, gout)
    sd = max(1, int(lib.nnl_linear_ce_bf16_bwd_workspace_bytes(M, N, K, 1, 0)) // (M * K * 4))
    sw = max(1, int(lib.nnl_linear_ce_bf16_bwd_workspace_bytes(M, N, K, 0, 1)) // (N * K * 4))
    assert (r['ranges'], sd) == (6, 3) or (M, N, K) != (40, 1300, 24), 'the range / dx-slab case lost its ranges or slabs'
    assert sw == 3 or (M, N, K) != (1300, 24, 40), 'the dw case lost its M slabs'
    flag = ops.index_error_flag(torch.device(DEV, torch.cuda.current_device()))
    flag.zero_()
    target = r['target'].to(DEV)
    runs = []
    for _ in range(2):
        x, w = r['x'].to(DEV).requires_grad_(True), r['w'].to(DEV).requires_grad_(True)
        loss = ops.linear_cross_entropy_bf16(x, w, target)
        loss.backward(torch.tensor(gout, device=DEV))
        runs.append((loss.detach(), x.grad, w.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'two calls on the same inputs differ'
    assert int(flag.item()) == (kind == 'bad'), 'the index-error flag'
    flag.zero_()
    x, w = r['x'].to(DEV), r['w'].to(DEV)                               # the C entry once more, for the row losses
    lse, rows, mean = torch.empty(M, device=DEV), torch.empty(M, device=DEV), torch.empty((), device=DEV)
    wsb = int(lib.nnl_linear_ce_bf16_fwd_workspace_bytes(M, N, K))
    ws = torch.empty(wsb // 4, device=DEV)
    assert lib.nnl_linear_ce_bf16_fwd(ptr(x), ptr(w), ptr(target), ptr(lse), ptr(rows), ptr(mean), M, N, K, K, K, ptr(ws), wsb, None, None) == 0
    assert torch.equal(mean, runs[0][0]), 'the op and the C entry disagree'
    bounded('loss rows, %d ranges' % r['ranges'], rows, r['loss'], r['loss_bound'] / U, 1)
    bounded('loss mean', runs[0][0], r['loss'].mean(), (r['loss_bound'].mean() + M * U * r['loss'].abs().mean()) / U, 1)
    _grad_bounded('dx', runs[0][1], r['dx'], r, r['w64'], N + sd + 2)
    _grad_bounded('dw', runs[0][2], r['dw'], r, r['x64'], M + sw + 2)
    assert runs[0][2].stride() == w.stride()


def test_c_entries_domain_and_refusals():
    M, N, K = 40, 1300, 24
    sup = lib.nnl_linear_ce_bf16_supported
    assert sup(M, N, K) and sup(1, 1, 512) and not sup(M, N, 513) and not sup(0, N, K) and not sup(M, 0, K) and not sup(M, N, 0)
    x, w, t = torch.randn(M, K, device=DEV), torch.randn(N, K, device=DEV), torch.zeros(M, dtype=torch.long, device=DEV)
    g = torch.ones(1, device=DEV)
    fb, bb = int(lib.nnl_linear_ce_bf16_fwd_workspace_bytes(M, N, K)), int(lib.nnl_linear_ce_bf16_bwd_workspace_bytes(M, N, K, 1, 1))
    assert fb > 0 and bb > 0 and int(lib.nnl_linear_ce_bf16_bwd_workspace_bytes(3, 5, 7, 1, 1)) == 0
    ws = torch.full((max(fb, bb) // 4,), 7.0, device=DEV)
    lse, rows, mean, dx, dw = (torch.full(s, 7.0, device=DEV) for s in ((M,), (M,), (1,), (M, K), (N, K)))
    fwd = lambda **k: lib.nnl_linear_ce_bf16_fwd(k.get('x', ptr(x)), ptr(w), k.get('t', ptr(t)), ptr(lse), ptr(rows), ptr(mean), M, N, k.get('K', K),   # noqa: E731
                                                 k.get('ldx', K), k.get('ldw', K), k.get('ws', ptr(ws)), k.get('wsb', fb), None, None)
    bwd = lambda **k: lib.nnl_linear_ce_bf16_bwd(ptr(x), k.get('w', ptr(w)), ptr(t), k.get('lse', ptr(lse)), ptr(g), ptr(dx), ptr(dw), M, N,          # noqa: E731
                                                 k.get('K', K), k.get('ldx', K), k.get('ldw', K), k.get('ws', ptr(ws)), k.get('wsb', bb), None)
    refused = {'null pointer': [fwd(x=None), fwd(t=None), bwd(w=None), bwd(lse=None)], 'short stride': [fwd(ldx=K - 1), fwd(ldw=K - 1), bwd(ldx=K - 1), bwd(ldw=K - 1)],
               'short workspace': [fwd(wsb=fb - 4), bwd(wsb=bb - 4)], 'null workspace': [fwd(ws=None), bwd(ws=None)],
               'K > 512': [fwd(K=513, ldx=513, ldw=513), bwd(K=513, ldx=513, ldw=513)]}
    for what, codes in refused.items():
        assert all(c != 0 for c in codes), what + ' accepted'
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in (ws, lse, rows, mean, dx, dw)), 'a refused call wrote'
    with pytest.raises(NotImplementedError, match='domain'):
        ops.linear_cross_entropy_bf16(torch.zeros(2, 513, device=DEV), torch.zeros(3, 513, device=DEV), t[:2])
