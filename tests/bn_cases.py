"""The case table of the BatchNorm C-ABI sweep (tests/test_bn_abi_gpu.py, tests/test_bn_cases_cpu.py) and its fp64 reference.

A plain module: no fixtures, nothing from the library.  The reference restates, in torch fp64, the formulas in the header comments of
nnl_bn_fwd / nnl_bn_bwd, the nnl_bn_sync_* entries and nnl_bn_relu_maxpool_* (include/nnl.h); tests/test_bn_cases_cpu.py holds it
against torch.nn.functional.batch_norm under autograd.

csrc/batchnorm.hip picks its loops from a host plan: make_shape (lanes L along the channel groups, rows per block iteration rpb, grid
gx x gy with gx clamped to kMaxRowBlocks / gy), ew_grid (elementwise blocks: a multiple of `unit`, about 8192 at most) and bnpool_grid.
Every case below exists for a regime of those loops and names it; facts() derives, from what nnl_debug_bn_plan reports, how often each
loop runs, REGIMES holds the predicates, and the CPU test checks every claim and that no regime is left without a case.

Data modes:
  int     x integer-valued in [-4, 4], dy in [-3, 3].  With the pivot K = x[0][c] every shifted difference is at most 8 in magnitude
          and its square at most 64, so up to 262144 rows sum(x-K), sum((x-K)^2) and sum(dy) stay below 2^24: exact in fp32 in ANY
          summation order (the library is built with -ffp-contract=off).  A reduction that drops or repeats one row is then off by an
          integer, not by a rounding.
  randn   x = 1.7 * randn + offset (offset 0 or 40: |mean| >> std), the tolerances of tests/test_bn_gpu.py and tests/test_pool_gpu.py.
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                                   # unit roundoff of fp32 (round to nearest)
EPS = 1e-5
EPS32 = float(np.float32(EPS))                   # what the kernels add to the variance: the float argument
MOMENTUM = 0.1
MOM32 = float(np.float32(MOMENTUM))
INT_MAX_ROWS = 262144                            # 64 * rows < 2^24

# the project's tolerances (rtol, atol): tests/test_bn_gpu.py::test_bn_act; *_REL: atol = that factor * max|reference|
TOL_Y = (1e-4, 1e-5)
TOL_DX = (1e-3, 1e-5)                            # atol = 1e-5 * max|dx| + 1e-7
TOL_DPARAM = (1e-3, 1e-4)                        # atol = 1e-4 * max|ref|
TOL_RMEAN = (1e-5, 1e-5)
TOL_RVAR = (1e-4, 1e-6)
TOL_STEM_DPARAM = (2e-3, 2e-3)                   # tests/test_pool_gpu.py: dgamma vs torch
TOL_STEM_AGREE = (1e-4, 1e-4)                    # tests/test_pool_gpu.py: two routes to the same dgamma / dbeta

Case = collections.namedtuple('Case', 'rows C regimes')


# ---- what the kernels do under a plan ------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


Facts = collections.namedtuple('Facts', 'rows C VEC CG L rpb gx gy capped cap ew_blocks ew_unit ew_passes ew_capped k_set fin_unrolled '
                                        'fin_tail mask_tail')


def facts(rows, C, plan):
    """plan = the ten values of nnl_debug_bn_plan.  k_set: the numbers of rows the thread slots of bn_stats_kernel / bn_bwd_reduce_kernel
    own (slot r0 in [0, gx*rpb) takes rows r0, r0 + gx*rpb, ...): the 4-way loop runs k // 4 times and leaves k % 4 rows, the 2-way loop
    k // 2 and k % 2.  fin_unrolled / fin_tail: the same for lane 0 of reduce_partials<64> over gx partials (8-way)."""
    VEC, L, rpb, gx, gy, capped, ew, cap = plan[:8]
    CG = C // VEC
    rstep = gx * rpb
    # k(r0) = ceil((rows - r0) / rstep) falls by at most one over the slots that own a row: the first and the last of them give the set
    k_set = frozenset((cdiv(rows, rstep), cdiv(rows - (min(rstep, rows) - 1), rstep)))
    total_v = rows * CG
    unit = CG // math.gcd(CG, 256)
    per_lane = cdiv(gx, 64)
    return Facts(rows, C, VEC, CG, L, rpb, gx, gy, bool(capped), cap, ew, unit, cdiv(total_v, ew * 256), cdiv(total_v, 512) > 8192,
                 k_set, per_lane // 8, per_lane % 8, total_v % 64)


def _k(f, passes=None, tails=None, div=4):
    return (passes is None or {k // div for k in f.k_set} == set(passes)) and (tails is None or {k % div for k in f.k_set} == set(tails))


REGIMES = collections.OrderedDict([
    ('rows < rpb', lambda f: f.rows < f.rpb),
    ('CG not a power of two', lambda f: f.CG & (f.CG - 1) != 0),
    ('n = 1', lambda f: f.rows == 1),
    ('tail-only loops, L = 64', lambda f: f.L == 64 and _k(f, passes=[0])),
    ('gy = 16', lambda f: f.gy == 16 and not f.capped),
    ('odd C', lambda f: f.VEC == 1 and f.C % 2 == 1),
    ('last finalize block partly empty', lambda f: f.C % 4 != 0),
    ('one unrolled pass plus a 3-row tail, L = 4', lambda f: f.L == 4 and f.k_set == {3, 4}),
    ('one unrolled pass plus a 3-row tail, L = 32', lambda f: f.L == 32 and f.k_set == {3, 4}),
    ('one unrolled pass plus a 3-row tail, L = 2', lambda f: f.L == 2 and f.k_set == {3, 4}),
    ('tabular layer, gy = 4', lambda f: f.gy == 4 and not f.capped and f.C == 1000),
    ('gx = 1024 uncapped', lambda f: f.gx == f.cap == 1024 and f.gy == 1 and not f.capped),
    ('reduce_partials<64> unrolled twice', lambda f: f.fin_unrolled == 2),
    ('capped, gx = 113, gy = 9', lambda f: f.capped and f.gx == 113 and f.gy == 9),
    ('two unrolled passes plus tail', lambda f: _k(f, passes=[2]) and any(k % 4 for k in f.k_set)),
    ('VEC = 1', lambda f: f.VEC == 1),
    ('elementwise unit = 513', lambda f: f.ew_unit == 513 and f.ew_blocks % 513 == 0),
    ('elementwise grid capped: 8208 blocks, 3 passes', lambda f: f.ew_capped and f.ew_blocks == 8208 and f.ew_passes == 3 and 8192 % f.ew_unit),
    ('4-5 unrolled passes', lambda f: _k(f, passes=[4, 5])),
    ('capped, gy = 8', lambda f: f.capped and f.gy == 8),
    ('capped, gy = 1', lambda f: f.capped and f.gy == 1 and f.gx == f.cap),
    # not in the issue's table, read off the same loops: the 2-way loop of bn_bwd_reduce_kernel with a second pass and a tail row
    ('bwd 2-way loop: several passes plus tail', lambda f: any(k // 2 >= 2 and k % 2 for k in f.k_set)),
    ('elementwise grid-stride loop: 2 passes', lambda f: f.ew_passes == 2),
] + [('mask tail %d' % t, (lambda f, t=t: f.mask_tail == t)) for t in (1, 18, 25, 39, 35, 45)])

CASES = [
    Case(1, 4, ['rows < rpb', 'n = 1', 'mask tail 1']),
    Case(3, 6, ['rows < rpb', 'CG not a power of two', 'mask tail 18', 'VEC = 1', 'last finalize block partly empty']),
    Case(5, 20, ['rows < rpb', 'CG not a power of two', 'mask tail 25']),
    Case(33, 7, ['CG not a power of two', 'mask tail 39', 'odd C']),
    Case(97, 3, ['CG not a power of two', 'mask tail 35', 'odd C']),
    Case(7, 256, ['tail-only loops, L = 64']),
    Case(37, 1001, ['gy = 16', 'odd C', 'last finalize block partly empty', 'mask tail 45']),
    Case(1025, 12, ['one unrolled pass plus a 3-row tail, L = 4']),
    Case(2049, 68, ['one unrolled pass plus a 3-row tail, L = 32']),
    Case(65539, 8, ['one unrolled pass plus a 3-row tail, L = 2']),
    Case(1024, 1000, ['tabular layer, gy = 4']),
    Case(16369, 256, ['gx = 1024 uncapped', 'reduce_partials<64> unrolled twice']),
    Case(16384, 256, ['gx = 1024 uncapped', 'reduce_partials<64> unrolled twice']),
    Case(4073, 513, ['capped, gx = 113, gy = 9', 'two unrolled passes plus tail', 'VEC = 1', 'elementwise unit = 513',
                     'bwd 2-way loop: several passes plus tail']),
    Case(9000, 513, ['elementwise grid capped: 8208 blocks, 3 passes', '4-5 unrolled passes']),
    Case(4625, 2048, ['capped, gy = 8', 'two unrolled passes plus tail']),
    Case(147493, 64, ['capped, gy = 1', 'two unrolled passes plus tail', 'elementwise grid-stride loop: 2 passes']),
]
SMALL = [c for c in CASES if c.rows * c.C <= 4096]


def case_id(c):
    return '%dx%d' % (c.rows, c.C)


# conv-epilogue partials: one (sum, sum of squares) pair per 64-row tile.  bn_finalize_kernel<64> below 1024 partials (its 8-way loop from
# 449 up: 1023 runs it twice), bn_finalize_kernel<256> from 1024 (tail only there; its 8-way loop from 1793 up)
EXT_TILE = 64
EXT_CASES = [(t, C) for t in (1, 63, 98, 1023, 1024, 1793, 3136) for C in (6, 64)]


def ext_rows_of(tiles):
    """the last tile is short (one row) wherever there is more than one tile"""
    return (tiles - 1) * EXT_TILE + (1 if tiles > 1 else EXT_TILE)


# the stem: (N, H, W, C, ks, stride, pad); odd H and W; the last one is large enough for a capped bnpool_grid (1024 blocks)
STEM_GEOMS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (1, 1, 0)]
STEM_CASES = [(2, 15, 13, C, ks, st, pd) for C in (4, 16, 64) for ks, st, pd in STEM_GEOMS] + \
             [(1, 7, 5, 1024, ks, st, pd) for ks, st, pd in STEM_GEOMS] + [(4, 257, 257, 64, 3, 2, 1)]
STEM_REFUSED_C = 12
STEM_REFUSAL = b'needs C % 4 == 0 and C/4 dividing 256'


def pool_out(H, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1


# SyncBN: (C, rows per rank).  65539 = 1 * 65536 + 3 travels with hi != 0
SYNC_CASES = [(8, [65539]), (6, [33]), (8, [1, 65539]), (7, [97, 1]), (12, [5, 1, 1025]), (8, [65539, 3, 70001])]


# ---- data ------------------------------------------------------------------------------------------------------------------------
def make_data(rows, C, mode, offset=0.0, seed=0):
    """fp32 CPU tensors x, dy, res [rows, C]; gamma, beta, rmean, rvar [C]"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + rows % 997)
    if mode == 'int':
        assert rows <= INT_MAX_ROWS
        x = torch.randint(-4, 5, (rows, C), generator=g).float()
        dy = torch.randint(-3, 4, (rows, C), generator=g).float()
    else:
        x = torch.randn(rows, C, generator=g) * 1.7 + offset
        dy = torch.randn(rows, C, generator=g)
    res = torch.randn(rows, C, generator=g)
    gamma = torch.randn(C, generator=g) * 0.3 + 1
    beta = torch.randn(C, generator=g) * 0.3
    rmean = torch.randn(C, generator=g) * 0.1 + offset
    rvar = torch.rand(C, generator=g) + 0.5
    return dict(x=x, dy=dy, res=res, gamma=gamma, beta=beta, rmean=rmean, rvar=rvar)


# ---- the fp64 reference (include/nnl.h, "K2: BatchNorm fused with the residual add and ReLU") ---------------------------------------------
def batch_stats(x):
    """biased batch statistics of x [rows, C] (fp64)"""
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def running_update(running, batch, momentum):
    return (1 - momentum) * running + momentum * batch


def unbiased(var, n):
    return var * (n / (n - 1.0)) if n > 1 else var


def bn_fwd_ref(x, gamma, beta, residual, mean, var, eps, relu):
    """y = (x-mean)*invstd*gamma + beta [+ residual] [ReLU]; returns (y, invstd)"""
    invstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * invstd
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    if residual is not None:
        y = y + residual
    return (torch.relu(y) if relu else y), invstd


def bn_bwd_ref(dy, gate, x, gamma, mean, invstd, training, n=None, sums=None):
    """g = dy * gate; dbeta = sum g; dgamma = sum g*xhat; dres = g; dx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n) (training) or
    gamma*invstd*g (eval).  n / sums: the global row count and (dbeta, dgamma) of a cross-replica batch (dx uses those)."""
    g = dy if gate is None else dy * gate
    xhat = (x - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    a = invstd if gamma is None else gamma * invstd
    if training:
        s1, s2 = (dbeta, dgamma) if sums is None else sums
        n = x.shape[0] if n is None else n
        dx = a * (g - s1 / n - xhat * (s2 / n))
    else:
        dx = a * g
    return dict(dx=dx, dres=g, dgamma=dgamma, dbeta=dbeta)


# ---- int mode: the header's expressions from exact sums, and the fp32 roundings they cost ----------------------------------------------
def shifted_sums(x, pivot):
    d = x - pivot
    return d.sum(0), (d * d).sum(0)


def stats_from_sums(S1, S2, pivot, n, rmean=None, rvar=None, momentum=MOM32, eps=EPS32):
    """What bn_finalize_kernel evaluates — m = K + S1/n, var = max((S2 - S1*(S1/n))/n, 0), invstd = 1/sqrt(var + eps), running =
    (1-momentum)*running + momentum*{m, var*n/(n-1)} — in fp64, with a bound on what its fp32 evaluation may differ by.  S1, S2, K, n
    enter exactly (int mode), every fp32 operation is correctly rounded (relative error <= U = 2^-24; hipcc's default for / and sqrt),
    so the bound is a count of roundings; the factor 1.01 covers the products of two such errors.
      m:       q = fl(S1/n), m = fl(K + q)                                     |dm|   <= U*(|q| + |m|)
      var:     b = fl(S1*q) carries 2 roundings, c = fl(S2 - b), v = fl(c/n)   |dv|   <= U*(2*q^2 + 2*v)        (b/n = q^2, c/n = v)
      invstd:  t = fl(v + eps), s = sqrt(t), is = fl(1/s): d(is)/is = -dt/2t   |dis|  <= is*(|dv|/(2t) + 2.5*U)
      running: e = fl(1 - mom), fl(fl(e*r) + fl(mom*z)) for z = m or the unbiased variance z = fl(v * fl(n/(n-1))) (2 more roundings)
                                                                              |dr'|  <= U*(2|(1-mom)r| + |mom z| + |r'|) + mom*|dz|"""
    q = S1 / n
    m = pivot + q
    v = torch.clamp((S2 - S1 * q) / n, min=0)
    t = v + eps
    inv = 1.0 / torch.sqrt(t)
    slack = 1.01
    out = dict(mean=m, var=v, invstd=inv)
    out['mean_bound'] = slack * U * (q.abs() + m.abs())
    dv = slack * U * (2 * q * q + 2 * v)
    out['var_bound'] = dv
    out['invstd_bound'] = slack * inv * (dv / (2 * t) + 2.5 * U)
    if rmean is not None:
        r = (1 - momentum) * rmean + momentum * m
        out['rmean'] = r
        out['rmean_bound'] = slack * (U * (2 * ((1 - momentum) * rmean).abs() + (momentum * m).abs() + r.abs()) + momentum * out['mean_bound'])
    if rvar is not None:
        z = unbiased(v, n)
        dz = (dv * (n / (n - 1.0)) if n > 1 else dv) + 2 * U * z
        r = (1 - momentum) * rvar + momentum * z
        out['rvar'] = r
        out['rvar_bound'] = slack * (U * (2 * ((1 - momentum) * rvar).abs() + (momentum * z).abs() + r.abs()) + momentum * dz)
    return out


def within(got, want, bound):
    """every element of got (fp32) within bound of want (fp64)"""
    return bool(((got.double() - want).abs() <= bound).all())


def worst(got, want, bound):
    err = (got.double() - want).abs()
    i = int((err - bound).argmax())
    return 'worst channel %d: got %r, want %r, |diff| %.3e, bound %.3e' % (i, got[i].item(), want[i].item(), err[i].item(), bound[i].item())


# ---- SyncBN (include/nnl.h, "Cross-replica (synchronised) training-mode BatchNorm") -----------------------------------------------------
def sync_local_ref(x):
    """stats of one rank: mean_r, M2_r = sum (x - mean_r)^2, hi, lo"""
    mean = x.mean(0)
    n = x.shape[0]
    return mean, ((x - mean) ** 2).sum(0), float(n >> 16), float(n & 0xFFFF)


# ---- the stem: BatchNorm -> ReLU -> MaxPool2d ---------------------------------------------------------------------------------------------------
def stem_forward_fp32(x, scale, shift, ks, stride, pad):
    """From the kernel's own save_scale / save_shift: z = relu(x*scale + shift) in fp32 (the kernel's two operations, uncontracted), pooled
    by torch with its tie rule.  x [N,H,W,C] fp32 -> (z [N,H,W,C], y [N,P,Q,C], idx [N,P,Q,C] = kh*ks + kw as uint8)."""
    N, H, W, C = x.shape
    z = torch.relu(x * scale + shift)
    y, ind = F.max_pool2d(z.permute(0, 3, 1, 2), ks, stride, pad, return_indices=True)
    P, Q = y.shape[2], y.shape[3]
    h, w = ind // W, ind % W
    kh = h - (torch.arange(P).view(1, 1, P, 1) * stride - pad)
    kw = w - (torch.arange(Q).view(1, 1, 1, Q) * stride - pad)
    idx = (kh * ks + kw).to(torch.uint8)
    return z, y.permute(0, 2, 3, 1).contiguous(), idx.permute(0, 2, 3, 1).contiguous()


def stem_scatter(dpool, idx, z, H, W, ks, stride, pad):
    """g [N,H,W,C] (fp64): every pooled gradient goes to the input position its idx names, gated by z > 0"""
    N, P, Q, C = dpool.shape
    t = idx.long()
    h = torch.arange(P).view(1, P, 1, 1) * stride - pad + t // ks
    w = torch.arange(Q).view(1, 1, Q, 1) * stride - pad + t % ks
    assert bool(((h >= 0) & (h < H) & (w >= 0) & (w < W)).all()), 'idx names a position outside the image'
    row = (torch.arange(N).view(N, 1, 1, 1) * H + h) * W + w
    g = torch.zeros(N * H * W, C, dtype=torch.float64)
    g.scatter_add_(0, row.view(-1, C), dpool.double().view(-1, C))
    return g.view(N, H, W, C) * (z > 0)


if __name__ == '__main__':
    for c in CASES:
        print(case_id(c), '; '.join(c.regimes))
