"""The case tables of the text-loss C-ABI sweep (tests/test_text_abi_gpu.py, tests/test_text_cases_cpu.py) and their fp64 references.

A plain module: no fixtures, nothing from the library.  It covers the nine entry points of csrc/text.hip: nnl_softmax_ce_fwd / _bwd,
nnl_embedding_rowmask_fwd / _bwd (+ workspace query), nnl_seq_reg_fwd / _bwd (+ workspace query) and nnl_weight_drop.  Every case exists
for a regime of a kernel's loops and names it; the *_facts() functions derive the regime from the sizes (and, for the embedding, from the
index vector) alone, the *_REGIMES tables hold the predicates, and the CPU test checks every claim and that no regime is left without a
case.  U = 2^-24.

Softmax-CE (block 256; the unrolled loop runs while v + 768 < V, the tail strides by 256; row_stats = {m, log s}).  With m, s*, p* from
fp64, L = the loop iterations of the busiest lane (ce_stages(): ceil(V / 256) without the unrolled loop, which takes four columns
at once) and E = sum_v p*_v (m - x_v) (the mean distance to the maximum: shift-invariant):
  log s      U (c4 + 2 |log s*|),  c4 = E + 2 + (L + 9 [+ 2]) + 3 (C + 9).  Every term exp(x - m) reaches s through at most L lane steps, 6
             butterfly merges and 3 merges across the waves: one addition each (+ 2 with the unrolled loop, whose four terms are added by
             a tree of depth 2 first).  A merge rescales by an expf (2U) and a multiply; a lane step does so only where the lane's running
             maximum rises (expf(0) = 1 and s * 1 are exact), at most C times (ce_max_changes(), counted from the logits).  The term's
             own expf is 2U.  (First count: 4 (L + 9), a rescale at every step; at V = 47343 that was 234U against a measured 1U.)
             The arguments of all the expf on a term's way are non-positive and add up to x - m, so their roundings add U |x - m| to the
             relative error of that term: E in the sum.  logf: 2U |log s|.
  loss_rows  log s bound + U (|x_t - m| + |loss*|): the difference x_t - m and the final subtraction round once each.  This is below
             c1 U (1 + |log s*| + |x_t - m|) with c1 = c4.
  dlogits    |g| / rows * (p* (U (4 + |x - m| + |log p*|) + log s bound) + 3U |p* - [v == t]| + 2^-126): x - m and (x - m) - log s round
             once each (absolute errors of the exponent), expf 2U, the subtraction of the onehot, g = grad_out / rows and the product 1U
             each, +1 slack; a p* below the normal range may come out as 0.
  mean       (ceil(rows / 256) + 10) U mean |loss_rows|, against the fp64 mean of the RETURNED loss_rows (chained, so that the bound is
             that of mean_kernel alone: ceil(rows/256) additions per thread, 8 tree levels, the division, +1).
  joined     for a row with |m| <= 16 the kernels form lse = fl(m + log s), loss = lse - x_t and p = exp(x - lse) (the bits of the kernels
             that stored lse alone: ordinary logits train exactly as before); that one rounding adds J = U (16 + |log s*|) to the bound of
             loss_rows and to the relative bound of p.  x - lse rounds by U |log p| like (x - m) - log s.  A constant, not |m|.
None of these contains |m| or |x|: the `offset` modes (all logits shifted by +-1000, +-20000) have the bounds of the unshifted row less J.
The `randn` and `masked` rows have |m| below 16 (the joined form), the `peaked` and `offset` rows above (test_text_cases_cpu.py checks).

Embedding row-mask.  Forward: out = fl(W[x] * rowmask[x]), bit for bit; an index outside [0, V) gives zeros and the flag.  Backward:
`int` mode (small integers, rowmask in {0, 1, 2}) is exact, so the sorted and the atomic path equal the reference bit for bit; `randn`
mode has U (len + 2) sum |term| per element, len = the samples of the row.

seq_reg (block 256, at most 1024 blocks, time loop unrolled by 8 from t = 1).  out3[1] / out3[2]: relative (A + 4) U / (A + 6) U with
A = T * passes + 8 + ceil(blocks / 256) + min(8, ceil(log2 blocks)) additions on the longest path (per thread, the block tree, per thread
of the final kernel, its tree: adding the zero of an idle thread is exact); the square 1U (a difference rounds 1U on d, so 2U more on
d^2), the scaling 1 / fl(T R) and the product 2U, +1.  `dyadic` mode (integers in [-2, 2], sums of squares exact below 2^24): 4U.
(First count: two trees of depth 8 whatever the number of blocks and 4U for the scaling, A + 21; t10 measured 0.008 of it.)
out3[0] against alpha * out3[1] + beta * out3[2] of the RETURNED values: 3U (|alpha a| + |beta t|).  dh elementwise:
|g| U (6 |ca h| + 8 |cb| (|h - h_prev| + |h_next - h|)), ca = 2 alpha / (T R), cb = 2 beta / ((T - 1) R).

weight_drop: out = fl(src * m) bit for bit, m the explicit mask or wd_keep() restated below (splitmix64 of seed + index * golden, top 24
bits, u >= p) times fl(1 / (1 - p)) formed in fp32.

Measured on an MI355X, max err / bound over the sweep (tests/test_text_abi_gpu.py prints them per case):
  softmax-CE  randn      log s 0.104   loss_rows 0.219   mean 0.132   dlogits 0.748     (joined form)
              peaked     log s 0.053   loss_rows 0.277   mean 0.078   dlogits 0.354
              offset     log s 0.084   loss_rows 0.122   mean 0.116   dlogits 0.656     (+-1000 and +-20000 together)
              masked     log s 0.095   loss_rows 0.159   mean 0.123   dlogits 0.555     (joined form; -inf columns: gradient exactly 0)
              nonfinite  log s 0.075   loss_rows 0.136                dlogits 0.479     (finite rows; NaN rows in the reference's places)
              bad target log s 0.039   loss_rows 0.172                dlogits 0.237
              smallest randn figure: log s 0.007 at V = 47343 (58 additions counted one after the other; the measured error is 1U)
  embedding   forward bit for bit; backward `int` bit for bit on the sorted and on the atomic path; `randn` 0.461 sorted, 0.322 atomic
  seq_reg     dyadic     out3[1] 0.201   out3[2] 0.229   out3[0] 0.332   dh 0.267
              randn      out3[1] 0.078   out3[2] 0.115   out3[0] 0.333   dh 0.465
              smallest randn figures: out3[2] 0.002 (t9), out3[1] 0.009 (t10): sums of thousands of squares, whose roundings average
              out, against a count of every addition on the longest path
  weight_drop bit for bit in every case; the kept share at most 1.37 standard deviations from 1 - p
  fp32 torch on the CPU (tests/test_text_cases_cpu.py) against the same softmax-CE bounds: log s 0.086, loss_rows 0.352, mean 0.165, dlogits 0.601
  The kernels before row_stats = {m, log s} (lse = fl(m + log s)): every `masked` case NaN, every `offset` case out of bound.
"""
import collections

import numpy as np

from optim_cases import U, _ratio, _same_bits, bits, cdiv

F32 = np.float32
NEG_INF = -np.inf
MAX_ELEMS = 4 * 1024 * 1024

# ======================================================================================================================================
# softmax-CE
# ======================================================================================================================================
CE_BLOCK = 256
CE_LSE_JOIN = 16.0                               # kLseJoin of csrc/text.hip: rows with |m| <= 16 form lse = m + log s
CE_MODES = ('randn', 'peaked', 'offset+1000', 'offset-1000', 'offset+20000', 'offset-20000', 'masked', 'nonfinite', 'badtarget')
CECase = collections.namedtuple('CECase', 'name rows V ld mode gout regimes')
CEFacts = collections.namedtuple('CEFacts', 'rows V ld unrolled0 tail0 lanes_unrolled max_tail busy_lanes mean_passes pad mode gout')


def ce_lane_steps(V, t):
    "(unrolled iterations, tail steps) of lane t in softmax_ce_fwd_kernel"
    v, un, tail = t, 0, 0
    while v + 3 * CE_BLOCK < V:
        v += 4 * CE_BLOCK
        un += 1
    while v < V:
        v += CE_BLOCK
        tail += 1
    return un, tail


def ce_stages(V):
    "the most loop iterations (unrolled + tail) any lane of the forward kernel takes: each rescales and adds once"
    return max(sum(ce_lane_steps(V, t)) for t in range(min(V, CE_BLOCK)))


def ce_max_changes(x64):
    """per row: the most often the running maximum of a lane rises after the lane's first column (lane t reads columns t, t + 256, ...).
    Only then does the lane rescale its sum by something other than expf(0) = 1.  Counted from the logits alone, column by column (the
    unrolled loop takes four columns in one step, so it rescales no more often)."""
    rows, V = x64.shape
    n = cdiv(V, CE_BLOCK)
    pad = np.full((rows, n * CE_BLOCK), NEG_INF)
    pad[:, :V] = np.where(np.isnan(x64), NEG_INF, x64)
    run = np.maximum.accumulate(pad.reshape(rows, n, CE_BLOCK), axis=1)
    return (run[:, 1:] > run[:, :-1]).sum(axis=1).max(axis=1) if n > 1 else np.zeros(rows)


def ce_ld(V, kind):
    return {'V': V, 'V+1': V + 1, 'ceil16': cdiv(V, 16) * 16}[kind]


def ce_facts(case):
    steps = [ce_lane_steps(case.V, t) for t in range(CE_BLOCK)]
    return CEFacts(case.rows, case.V, ce_ld(case.V, case.ld), steps[0][0], steps[0][1], sum(1 for s in steps if s[0] > 0),
                   max(s[1] for s in steps), min(case.V, CE_BLOCK), cdiv(case.rows, CE_BLOCK), ce_ld(case.V, case.ld) - case.V,
                   case.mode, case.gout)


CE_REGIMES = collections.OrderedDict([
    ('V = 1', lambda f: f.V == 1),
    ('V < 64: one wave partly idle', lambda f: 1 < f.V < 64),
    ('64 <= V < 256: idle lanes merge with s == 0', lambda f: 64 <= f.V < 256),
    ('V = 256', lambda f: f.V == 256 and f.unrolled0 == 0 and f.max_tail == 1),
    ('V = 257: tail only, lane 0 alone takes a second step', lambda f: f.V == 257 and f.unrolled0 == 0 and f.tail0 == 2),
    ('tail only, 2 steps', lambda f: 257 < f.V <= 512 and f.lanes_unrolled == 0 and f.tail0 == 2),
    ('tail only, 3 steps', lambda f: 512 < f.V <= 768 and f.lanes_unrolled == 0 and f.tail0 == 3),
    ('V = 768: the unrolled loop just not entered', lambda f: f.V == 768 and f.lanes_unrolled == 0),
    ('V = 769: only lane 0 enters the unrolled loop', lambda f: f.V == 769 and f.lanes_unrolled == 1 and f.tail0 == 0),
    ('V = 1024', lambda f: f.V == 1024 and f.lanes_unrolled == 256 and f.max_tail == 0),
    ('V = 1025', lambda f: f.V == 1025 and f.unrolled0 == 1 and f.tail0 == 1),
    ('two unrolled iterations, no tail', lambda f: f.unrolled0 == 2 and f.lanes_unrolled == 256 and f.max_tail == 0),
    ('two unrolled iterations, three tail steps', lambda f: f.unrolled0 == 2 and f.tail0 == 3),
    ('V = 47343, 4 rows', lambda f: f.V == 47343 and f.rows == 4),
    ('rows = 1', lambda f: f.rows == 1),
    ('rows = 7', lambda f: f.rows == 7),
    ('rows = 300: mean_kernel strides twice', lambda f: f.rows == 300 and f.mean_passes == 2),
    ('ld = V', lambda f: f.pad == 0),
    ('ld = V + 1', lambda f: f.pad == 1),
    ('ld = V rounded up to 16, several pad columns', lambda f: f.ld % 16 == 0 and f.pad > 1),
    ('grad_out = 1', lambda f: f.gout == 1.0),
    ('grad_out = 2.5', lambda f: f.gout == 2.5),
] + [('mode ' + m, (lambda m: lambda f: f.mode == m)(m)) for m in CE_MODES])


def _ce(name, rows, V, ld, mode, gout, *regimes):
    f = ['rows = %d' % rows if rows != 300 else 'rows = 300: mean_kernel strides twice'] if rows in (1, 7, 300) else []
    f.append({'V': 'ld = V', 'V+1': 'ld = V + 1', 'ceil16': 'ld = V rounded up to 16, several pad columns'}[ld])
    f += ['grad_out = %g' % gout, 'mode ' + mode]
    return CECase(name, rows, V, ld, mode, gout, list(regimes) + f)


_T2, _T3 = 'tail only, 2 steps', 'tail only, 3 steps'
CE_CASES = [
    _ce('v1', 7, 1, 'ceil16', 'randn', 1.0, 'V = 1'),
    _ce('v1-off', 1, 1, 'V', 'offset+20000', 2.5, 'V = 1'),
    _ce('v10', 7, 10, 'ceil16', 'randn', 2.5, 'V < 64: one wave partly idle'),
    _ce('v37-masked', 7, 37, 'V+1', 'masked', 1.0, 'V < 64: one wave partly idle'),
    _ce('v200', 300, 200, 'V', 'randn', 1.0, '64 <= V < 256: idle lanes merge with s == 0'),
    _ce('v65-masked', 7, 65, 'ceil16', 'masked', 2.5, '64 <= V < 256: idle lanes merge with s == 0'),
    _ce('v200-off', 7, 200, 'V+1', 'offset-1000', 1.0, '64 <= V < 256: idle lanes merge with s == 0'),
    _ce('v256', 7, 256, 'V', 'peaked', 2.5, 'V = 256'),
    _ce('v256-masked', 7, 256, 'V+1', 'masked', 1.0, 'V = 256'),
    _ce('v257', 7, 257, 'ceil16', 'randn', 1.0, 'V = 257: tail only, lane 0 alone takes a second step'),
    _ce('v300', 300, 300, 'ceil16', 'randn', 2.5, _T2),
    _ce('v300-masked', 7, 300, 'V+1', 'masked', 2.5, _T2),
    _ce('v300-off+1000', 7, 300, 'V', 'offset+1000', 1.0, _T2),
    _ce('v300-off+20000', 7, 300, 'ceil16', 'offset+20000', 2.5, _T2),
    _ce('v300-nonfinite', 7, 300, 'V+1', 'nonfinite', 1.0, _T2),
    _ce('v300-badtarget', 7, 300, 'ceil16', 'badtarget', 2.5, _T2),
    _ce('v512', 1, 512, 'V', 'peaked', 1.0, _T2),
    _ce('v513', 7, 513, 'V+1', 'randn', 1.0, _T3),
    _ce('v700-masked', 7, 700, 'ceil16', 'masked', 1.0, _T3),
    _ce('v768', 7, 768, 'V', 'offset-20000', 1.0, 'V = 768: the unrolled loop just not entered', _T3),
    _ce('v769', 7, 769, 'ceil16', 'randn', 2.5, 'V = 769: only lane 0 enters the unrolled loop'),
    _ce('v769-masked', 7, 769, 'V', 'masked', 1.0, 'V = 769: only lane 0 enters the unrolled loop'),
    _ce('v1024', 7, 1024, 'V', 'randn', 1.0, 'V = 1024'),
    _ce('v1024-masked', 7, 1024, 'V+1', 'masked', 2.5, 'V = 1024'),
    _ce('v1025', 7, 1025, 'ceil16', 'peaked', 1.0, 'V = 1025'),
    _ce('v1500-off', 7, 1500, 'V+1', 'offset-1000', 2.5),
    _ce('v2048', 7, 2048, 'V', 'offset+1000', 2.5, 'two unrolled iterations, no tail'),
    _ce('v2815', 7, 2815, 'V+1', 'randn', 1.0, 'two unrolled iterations, three tail steps'),
    _ce('v2815-masked', 7, 2815, 'V', 'masked', 1.0, 'two unrolled iterations, three tail steps'),
    _ce('v2815-nonfinite', 7, 2815, 'V', 'nonfinite', 2.5, 'two unrolled iterations, three tail steps'),
    _ce('v47343', 4, 47343, 'V+1', 'randn', 1.0, 'V = 47343, 4 rows'),                      # (V + 1 = 47344 is V rounded up to 16)
    _ce('v47343-off', 4, 47343, 'V', 'offset+20000', 2.5, 'V = 47343, 4 rows'),
]


def case_id(c):
    return c.name


def ce_data(case, seed=0):
    """fp32 logits [rows, V], int64 targets, the boolean mask of the -inf columns.  Targets cycle through column 0, column V - 1, the
    column of the row maximum and a random one (masked: the first / last finite column instead)."""
    r = np.random.RandomState(100 + seed + 7 * [c.name for c in CE_CASES].index(case.name) if case in CE_CASES else 99)
    rows, V, mode = case.rows, case.V, case.mode
    assert rows * ce_ld(V, case.ld) <= MAX_ELEMS
    x = 3.0 * r.randn(rows, V)
    if mode == 'peaked':
        x[np.arange(rows), (7 * np.arange(rows) + 3) % V] += 30.0
    if mode.startswith('offset'):
        x += float(mode[6:])
    x = x.astype(F32)
    masked = np.zeros((rows, V), dtype=bool)
    if mode == 'masked':
        for i in range(rows):
            k = i % 4
            if k == 0:                                                       # the first column that lanes 0, 1, 63, 64, 255 read, and the last one
                masked[i, [c for c in (0, 1, 63, 64, 255, V - 1) if c < V]] = True
            elif k == 1:                                                     # a whole stripe: the first value EVERY lane reads
                masked[i, :CE_BLOCK if V > CE_BLOCK else max(V // 2, 1)] = True
            elif k == 2:                                                     # all but one column
                masked[i, :] = True
            else:                                                            # the second stripe, or a random third
                if V > 2 * CE_BLOCK:
                    masked[i, CE_BLOCK:2 * CE_BLOCK] = True
                else:
                    masked[i] = r.rand(V) < 0.33
            keep = (5 * i + 2) % V if k != 1 else V - 1                      # one finite column at least
            masked[i, keep] = False
        x[masked] = NEG_INF
    if mode == 'nonfinite':
        assert rows >= 4 and V >= 4
        x[0, V // 3] = np.nan
        x[1, V // 2] = np.inf
        x[2, :] = NEG_INF
    t = np.zeros(rows, dtype=np.int64)
    for i in range(rows):
        fin = np.flatnonzero(np.isfinite(x[i]))
        if fin.size == 0:
            t[i] = i % V
            continue
        k = i % 4
        t[i] = (fin[0], fin[-1], fin[np.argmax(x[i, fin])], fin[r.randint(fin.size)])[k]
    if mode == 'badtarget':
        t[2], t[5] = -1, V
    return x, t, masked


def ce_reference(x, t, gout):
    """fp64: m (the maximum, NaN ignored as fmaxf does), log s, loss_rows (0 for a target outside [0, V)), mean over ALL rows, p,
    dlogits = (p - onehot) * gout / rows (a row with a bad target has no onehot), and the bounds of the module docstring."""
    x64 = x.astype(np.float64)
    rows, V = x64.shape
    with np.errstate(all='ignore'):
        m = np.fmax.reduce(x64, axis=1)
        z = np.where(m == NEG_INF, 0.0, m)                                  # (a row of -inf: s = 0, log s = -inf, loss NaN)
        s = np.exp(x64 - z[:, None]).sum(axis=1)
        logs = np.log(s)
        xm = x64 - m[:, None]
        logp = xm - logs[:, None]
        p = np.exp(logp)
        ok = (t >= 0) & (t < V)
        tt = np.where(ok, t, 0)
        xt_m = xm[np.arange(rows), tt]
        loss = np.where(ok, logs - xt_m, 0.0)
        onehot = np.zeros((rows, V))
        onehot[np.arange(rows)[ok], t[ok]] = 1.0
        g = float(gout) / rows
        d = (p - onehot) * g
        L, C = ce_stages(V), ce_max_changes(x64)
        E = np.where(p > 0, p * -xm, 0.0).sum(axis=1)
        c4 = E + 2 + (L + 9 + (2 if V > 3 * CE_BLOCK else 0)) + 3 * (C + 9)
        logs_bound = U * (c4 + 2 * np.abs(logs))
        J = U * np.where(np.abs(m) <= CE_LSE_JOIN, CE_LSE_JOIN + np.abs(logs), 0.0)       # the rounding of m + log s where the kernel joins them
        loss_bound = np.where(ok, logs_bound + J + U * (np.abs(xt_m) + np.abs(loss)), 0.0)
        rel = U * (4 + np.where(p > 0, np.abs(xm) + np.abs(logp), 0.0)) + (logs_bound + J)[:, None]
        d_bound = abs(g) * (p * rel + 3 * U * np.abs(p - onehot) + 2.0 ** -126)
    return dict(m=m, logs=logs, loss=loss, mean=loss.sum() / rows, p=p, d=d, logs_bound=logs_bound, loss_bound=loss_bound, d_bound=d_bound,
                ok=ok)


def mean_bound(loss_rows):
    "of mean_kernel alone: against the fp64 mean of the fp32 loss_rows it was given"
    n = len(loss_rows)
    with np.errstate(all='ignore'):
        return (cdiv(n, CE_BLOCK) + 10) * U * np.abs(loss_rows.astype(np.float64)).sum() / n


def check_ce(case, x, t, masked, got, ctx=''):
    """got: dict(stats [rows, 2], loss_rows [rows], mean scalar, d [rows, ld], err_flag int).  Returns the ratios max err / bound."""
    ref = ce_reference(x, t, case.gout)
    rows, V = x.shape
    r = collections.OrderedDict()
    if got.get('stats') is not None:
        stats = np.asarray(got['stats'], dtype=F32).reshape(rows, 2)
        _same_bits(stats[:, 0], ref['m'].astype(F32), 'row maximum', ctx)
        r['logs'] = _ratio(stats[:, 1], ref['logs'], ref['logs_bound'], 'log s', ctx)
    r['loss'] = _ratio(got['loss_rows'], ref['loss'], ref['loss_bound'], 'loss_rows', ctx)
    lr = np.asarray(got['loss_rows'], dtype=F32)
    with np.errstate(all='ignore'):
        want_mean = lr.astype(np.float64).sum() / rows
    r['mean'] = _ratio([got['mean']], [want_mean], mean_bound(lr), 'mean', ctx)
    d = np.asarray(got['d'], dtype=F32)
    assert d.shape[0] == rows and d.shape[1] >= V
    assert not d[:, V:].any() and not np.signbit(d[:, V:]).any(), '%s: a pad column of dlogits is not +0' % ctx
    r['d'] = _ratio(d[:, :V].ravel(), ref['d'].ravel(), ref['d_bound'].ravel(), 'dlogits', ctx)
    if masked.any():
        assert not d[:, :V][masked].any(), '%s: a -inf logit has a gradient' % ctx
    assert int(got['err_flag']) == (0 if ref['ok'].all() else 1), '%s: err_flag %r' % (ctx, got['err_flag'])
    if not ref['ok'].all():
        assert not np.asarray(got['loss_rows'])[~ref['ok']].any(), '%s: loss of a row with a bad target is not 0' % ctx
    return r


def ce_result_from(ref, ld, rows, err=None):
    "the reference rounded to fp32, in the layout check_ce() takes"
    V = ref['d'].shape[1]
    d = np.zeros((rows, ld), dtype=F32)
    d[:, :V] = ref['d'].astype(F32)
    loss = ref['loss'].astype(F32)
    with np.errstate(all='ignore'):
        mean = F32(loss.astype(np.float64).sum() / rows)
    return dict(stats=np.stack([ref['m'], ref['logs']], axis=1).astype(F32), loss_rows=loss, mean=mean, d=d,
                err_flag=(0 if ref['ok'].all() else 1) if err is None else err)


# ======================================================================================================================================
# embedding with a vocabulary-row mask
# ======================================================================================================================================
EMB_MAX_SORT = 32768                             # nnl_det::kMaxSamples: above it the backward takes the atomic kernel
EMB_FWD_GRID = 4096 * 256                        # threads of the forward's largest grid
EmbCase = collections.namedtuple('EmbCase', 'name V D n pad rowmask invalid regimes')
EmbFacts = collections.namedtuple('EmbFacts', 'V D n DL SL lens last_len last_at_end has_invalid pad pad_is_top rowmask fwd_passes atomic d_loops')


def emb_dl_sl(D):
    DL = 1
    while DL < D and DL < 64:
        DL <<= 1
    return DL, 64 // DL


def emb_indices(case):
    """int64 indices [n]: row 0 once, row 1 SL times, row 2 SL + 1 times, row 3 70 times (as far as n allows), the top row V - 1 1 + 64 k
    times, the rest random over rows 4 .. V - 2, all at shuffled positions; with case.invalid, a few of the random ones become -1 and V."""
    r = np.random.RandomState(case.n * 31 + case.D)
    V, n = case.V, case.n
    _, SL = emb_dl_sl(case.D)
    x, left = [], n
    k = max((n // 3 - 1) // 64, 0)
    plan = [(V - 1, 1 + 64 * k if n >= 3 else 0), (0, 1), (1, SL), (2, SL + 1), (3, 70)]
    for row, cnt in plan:
        if 0 < cnt <= left and row < V:
            x += [row] * cnt
            left -= cnt
    if left:
        lo, hi = (4, V - 1) if V > 6 else (0, V)
        x += r.randint(lo, hi, left).tolist()
    x = np.asarray(x, dtype=np.int64)
    if case.invalid and left >= 4:
        x[n - 1], x[n - 2], x[n - 3] = -1, -1, V if case.invalid == 'both' else -1
    return x[r.permutation(n)] if n else x


def emb_pad_of(case, x):
    if case.pad == 'top':
        valid = x[(x >= 0) & (x < case.V)]
        return int(np.bincount(valid, minlength=case.V).argmax())
    return -1 if case.pad is None else int(case.pad)


def emb_facts(case):
    x = emb_indices(case)
    DL, SL = emb_dl_sl(case.D)
    valid = x[(x >= 0) & (x < case.V)]
    cnt = np.bincount(valid, minlength=case.V) if valid.size else np.zeros(case.V, dtype=np.int64)
    lens = sorted(set(int(c) for c in cnt if c > 0))
    top = int(x.max()) if x.size else -1
    last_len = int((x == top).sum()) if x.size else 0
    pad = emb_pad_of(case, x)
    return EmbFacts(case.V, case.D, case.n, DL, SL, lens, last_len, 0 <= top < case.V, bool(((x < 0) | (x >= case.V)).any()),
                    pad, pad >= 0 and cnt[pad] == cnt.max() and cnt.max() > 1, case.rowmask, cdiv(case.n * case.D, EMB_FWD_GRID),
                    case.n > EMB_MAX_SORT, cdiv(case.D, DL))


EMB_REGIMES = collections.OrderedDict(
    [('D = %d' % D, (lambda D: lambda f: f.D == D)(D)) for D in (1, 3, 8, 33, 64, 80, 400)] +
    [('n = %d' % n, (lambda n: lambda f: f.n == n)(n)) for n in (0, 1, 63, 64, 65, 4480)] + [
        ('n > 32768, D = 1: the atomic kernel', lambda f: f.atomic and f.D == 1),
        ('segment of length 1', lambda f: 1 in f.lens),
        ('segment of 2 .. SL samples', lambda f: any(1 < l <= f.SL for l in f.lens)),
        ('segment longer than SL', lambda f: any(f.SL < l <= 64 for l in f.lens)),
        ('segment longer than 64: a second ballot round', lambda f: any(l > 64 for l in f.lens)),
        ('last segment ends at the end of the array after 1 + 64 k positions',
         lambda f: f.last_at_end and f.last_len > 1 and f.last_len % 64 == 1 and not f.atomic),
        ('D > 64: two element passes per row', lambda f: f.d_loops == 2),
        ('D = 400: seven element passes, the last partial', lambda f: f.d_loops == 7),
        ('no padding_idx', lambda f: f.pad < 0),
        ('padding_idx', lambda f: f.pad >= 0 and not f.pad_is_top),
        ('padding_idx is the most frequent row', lambda f: f.pad_is_top),
        ('rowmask NULL', lambda f: not f.rowmask),
        ('rowmask with zeros', lambda f: f.rowmask),
        ('indices -1 and V among valid ones', lambda f: f.has_invalid and f.n > 4),
        ('forward grid-stride: n * D > 4096 * 256', lambda f: f.fwd_passes > 1),
    ])

_S1, _SS, _SG, _S64 = ('segment of length 1', 'segment of 2 .. SL samples', 'segment longer than SL',
                       'segment longer than 64: a second ballot round')
_LAST = 'last segment ends at the end of the array after 1 + 64 k positions'
EMB_CASES = [
    EmbCase('n0', 11, 8, 0, None, False, None, ['n = 0', 'D = 8', 'no padding_idx', 'rowmask NULL']),
    EmbCase('n1', 11, 3, 1, None, False, None, ['n = 1', 'D = 3', 'segment of length 1', 'rowmask NULL']),
    EmbCase('n63', 20, 33, 63, 2, True, None, ['n = 63', 'rowmask with zeros', 'D = 33', 'padding_idx', _S1, _SG]),
    EmbCase('n64', 20, 64, 64, None, False, None, ['n = 64', 'D = 64', _S1, _SG]),
    EmbCase('n65', 9, 80, 65, 'top', True, None, ['n = 65', 'D = 80', 'D > 64: two element passes per row',
                                                  'padding_idx is the most frequent row']),
    EmbCase('d1', 50, 1, 700, None, True, 'both', ['D = 1', 'rowmask with zeros', _S1, _SS, _S64, 'indices -1 and V among valid ones']),
    EmbCase('d3', 40, 3, 600, 7, False, 'neg', ['D = 3', _S1, _SS, _SG, _S64, _LAST]),
    EmbCase('d8', 40, 8, 500, None, True, 'both', ['D = 8', _S1, _SS, _SG, _S64]),
    EmbCase('d33', 30, 33, 400, None, False, None, ['D = 33', _S64, _LAST, 'no padding_idx', 'rowmask NULL']),
    EmbCase('lm', 977, 400, 4480, 1, True, 'both', ['n = 4480', 'D = 400', 'D = 400: seven element passes, the last partial',
                                                  'forward grid-stride: n * D > 4096 * 256', 'indices -1 and V among valid ones', _S64]),
    EmbCase('atomic', 50, 1, 40000, 3, True, 'both', ['n > 32768, D = 1: the atomic kernel', 'D = 1']),
]
EMB_MODES = ('int', 'randn')


def emb_data(case, mode):
    "x [n], W [V, D], rowmask [V] or None, dout [n, D], padding_idx"
    r = np.random.RandomState(case.V + case.D + (0 if mode == 'int' else 1000))
    x = emb_indices(case)
    V, D, n = case.V, case.D, case.n
    if mode == 'int':
        W, dout = r.randint(-4, 5, (V, D)), r.randint(-4, 5, (n, D))
        rm = r.randint(0, 3, V) if case.rowmask else None
    else:
        W, dout = r.randn(V, D), r.randn(n, D)
        rm = r.choice([0.0, 1.25, 0.7, 1.0 / 0.9], V) if case.rowmask else None
    if rm is not None:
        rm[x[(x >= 0) & (x < V)][:1]] = 0                                    # a zero on a row that is used
        rm = rm.astype(F32)
    return dict(x=x, W=W.astype(F32), rowmask=rm, dout=dout.astype(F32), pad=emb_pad_of(case, x), mode=mode)


def emb_fwd_ref(d):
    "(out fp32 — the fp64 product rounded once is the fp32 product — and the flag)"
    x, W = d['x'], d['W'].astype(np.float64)
    V = W.shape[0]
    ok = (x >= 0) & (x < V)
    xs = np.where(ok, x, 0)
    rm = np.ones(V) if d['rowmask'] is None else d['rowmask'].astype(np.float64)
    out = np.where(ok[:, None], W[xs] * rm[xs][:, None], 0.0)
    return out.astype(F32), int((~ok).any())


def emb_bwd_ref(d, drop_one_of_row=None, pad_gets_gradient=False):
    """fp64 dW [V, D] and the randn bound U (len + 2) sum |term|.  The two arguments build the mutants: one sample of a row left out; the
    padding row treated like any other."""
    x, dout = d['x'], d['dout'].astype(np.float64)
    V, D = d['W'].shape
    rm = np.ones(V) if d['rowmask'] is None else d['rowmask'].astype(np.float64)
    use = (x >= 0) & (x < V)
    if not pad_gets_gradient:
        use &= x != d['pad']
    if drop_one_of_row is not None:
        use[np.flatnonzero(use & (x == drop_one_of_row))[-1]] = False
    xs = x[use]
    term = dout[use] * rm[xs][:, None]
    dW, absum = np.zeros((V, D)), np.zeros((V, D))
    np.add.at(dW, xs, term)
    np.add.at(absum, xs, np.abs(term))
    cnt = np.bincount(xs, minlength=V).astype(np.float64)
    return dW, U * (cnt[:, None] + 2) * absum


def check_emb_bwd(d, got, ctx=''):
    dW, bound = emb_bwd_ref(d)
    if d['mode'] == 'int':
        assert np.abs(dW).max(initial=0) < 2 ** 24
        _same_bits(got, dW.astype(F32), 'dW', ctx)
        return 0.0
    return _ratio(np.ravel(got), dW.ravel(), bound.ravel(), 'dW', ctx)


# ======================================================================================================================================
# AR / TAR regulariser
# ======================================================================================================================================
REG_BLOCK, REG_MAX_BLOCKS = 256, 1024
REG_AB = ((2.0, 0.0), (0.0, 1.0), (2.0, 1.0))    # (alpha, beta): beta = 0, alpha = 0, both
REG_MODES = ('dyadic', 'randn')
RegCase = collections.namedtuple('RegCase', 'name T R regimes')
RegFacts = collections.namedtuple('RegFacts', 'T R blocks passes unrolled tail last_block_lanes')


def reg_facts(case):
    blocks = min(cdiv(case.R, REG_BLOCK), REG_MAX_BLOCKS)
    un = max(case.T - 1, 0) // 8
    return RegFacts(case.T, case.R, blocks, cdiv(case.R, blocks * REG_BLOCK), un, max(case.T - 1, 0) - 8 * un,
                    case.R - (cdiv(case.R, REG_BLOCK) - 1) * REG_BLOCK)


REG_REGIMES = collections.OrderedDict(
    [('T = %d' % T, (lambda T: lambda f: f.T == T)(T)) for T in (1, 2, 8, 9, 10, 17)] +
    [('R = %d' % R, (lambda R: lambda f: f.R == R)(R)) for R in (1, 255, 256, 257, 5000)] + [
        ('T = 1: no time step at all', lambda f: f.T == 1 and f.unrolled == 0 and f.tail == 0),
        ('tail only', lambda f: f.unrolled == 0 and f.tail > 0),
        ('T = 9: one unrolled pass, no tail', lambda f: f.unrolled == 1 and f.tail == 0),
        ('one unrolled pass and a tail', lambda f: f.unrolled == 1 and f.tail > 0),
        ('T = 17: two unrolled passes', lambda f: f.unrolled == 2 and f.tail == 0),
        ('R = 1024 * 256 + 300: the column loop runs a second pass', lambda f: f.R == 1024 * 256 + 300 and f.passes == 2 and f.T == 2),
        ('last block partly idle', lambda f: f.last_block_lanes < REG_BLOCK),
    ])
REG_CASES = [
    RegCase('t1', 1, 257, ['T = 1', 'R = 257', 'T = 1: no time step at all', 'last block partly idle']),
    RegCase('t2', 2, 1, ['T = 2', 'R = 1', 'tail only']),
    RegCase('t8', 8, 255, ['T = 8', 'R = 255', 'tail only', 'last block partly idle']),
    RegCase('t9', 9, 256, ['T = 9', 'R = 256', 'T = 9: one unrolled pass, no tail']),
    RegCase('t10', 10, 5000, ['T = 10', 'R = 5000', 'one unrolled pass and a tail']),
    RegCase('t17', 17, 257, ['T = 17', 'T = 17: two unrolled passes']),
    RegCase('wide', 2, 1024 * 256 + 300, ['R = 1024 * 256 + 300: the column loop runs a second pass']),
]


def reg_data(case, mode):
    r = np.random.RandomState(case.T * 1000 + case.R % 997)
    assert case.T * case.R <= MAX_ELEMS
    if mode == 'dyadic':
        h = r.randint(-2, 3, (case.T, case.R))
        assert 16 * case.T * case.R < 2 ** 24                               # sum h^2 <= 4 T R and sum d^2 <= 16 (T - 1) R: exact in fp32
    else:
        h = r.randn(case.T, case.R)
    return h.astype(F32)


def reg_reference(h, alpha, beta, g=1.0, seam_mutant=False):
    """fp64 out3[1], out3[2], dh and the bounds of the module docstring (rtol1, rtol2, dh_bound).  seam_mutant: the difference at t = 9
    taken against h[7] instead of h[8] (the `prev` of the first unrolled pass not carried into the second)."""
    h64 = h.astype(np.float64)
    T, R = h64.shape
    prev = np.vstack([h64[:1], h64[:-1]])
    if seam_mutant and T > 9:
        prev[9] = h64[7]
    dif = h64 - prev                                                        # dif[0] = 0
    ar = (h64 * h64).sum() / (T * R)
    tar = (dif[1:] ** 2).sum() / ((T - 1) * R) if T > 1 else 0.0
    ca = 2.0 * np.float64(F32(alpha)) / (T * R)
    cb = 2.0 * np.float64(F32(beta)) / ((T - 1) * R) if T > 1 else 0.0
    back = dif
    fwd = np.vstack([dif[1:], np.zeros((1, R))])                            # h[t+1] - h[t], 0 at the end
    dh = g * (ca * h64 + cb * (back - fwd))
    dh_bound = abs(g) * U * (6 * np.abs(ca * h64) + 8 * abs(cb) * (np.abs(back) + np.abs(fwd)))
    f = reg_facts(RegCase('', T, R, []))
    A = T * f.passes + 8 + cdiv(f.blocks, REG_BLOCK) + min(8, int(np.ceil(np.log2(f.blocks))))
    return dict(ar=ar, tar=tar, dh=dh, dh_bound=dh_bound, rtol1=(A + 4) * U, rtol2=(A + 6) * U)


def check_reg(h, alpha, beta, g, mode, out3, dh, ctx=''):
    ref = reg_reference(h, alpha, beta, g)
    T = h.shape[0]
    r = collections.OrderedDict()
    rt1, rt2 = (4 * U, 4 * U) if mode == 'dyadic' else (ref['rtol1'], ref['rtol2'])
    r['ar'] = _ratio([out3[1]], [ref['ar']], rt1 * ref['ar'], 'out3[1]', ctx)
    if T == 1:
        assert bits(out3[2]) == bits(F32(0.0)), '%s: T = 1 but out3[2] = %r' % (ctx, out3[2])
        r['tar'] = 0.0
    else:
        r['tar'] = _ratio([out3[2]], [ref['tar']], rt2 * ref['tar'], 'out3[2]', ctx)
    a, b, o1, o2 = (np.float64(F32(v)) for v in (alpha, beta, out3[1], out3[2]))
    r['value'] = _ratio([out3[0]], [a * o1 + b * o2], 3 * U * (abs(a * o1) + abs(b * o2)), 'out3[0]', ctx)
    if dh is not None:
        r['dh'] = _ratio(np.ravel(dh), ref['dh'].ravel(), ref['dh_bound'].ravel(), 'dh', ctx)
    return r


# ======================================================================================================================================
# weight drop
# ======================================================================================================================================
WD_GRID = 8192 * 256
WD_P = (0.25, 0.5, 0.9)
WD_SEEDS = (0, 1, 0x9E3779B97F4A7C15, 2 ** 62 - 57)
WDCase = collections.namedtuple('WDCase', 'name rows H ld_src ld_out kind p seed regimes')   # kind: 'mask', 'hash', 'copy'
WDFacts = collections.namedtuple('WDFacts', 'rows H ld_src ld_out pad kind p passes backward')


def wd_ld_out(H, kind):
    return {'H': H, 'H+1': H + 1, 'ceil32': cdiv(H, 32) * 32}[kind]


def wd_facts(c):
    ld_out = wd_ld_out(c.H, c.ld_out)
    return WDFacts(c.rows, c.H, c.ld_src, ld_out, ld_out - c.H, c.kind, c.p, cdiv(c.rows * ld_out, WD_GRID), c.ld_src > c.H and ld_out == c.H)


WD_REGIMES = collections.OrderedDict([
    ('explicit mask', lambda f: f.kind == 'mask'),
    ('ld_src > H', lambda f: f.ld_src > f.H),
    ('ld_out = H', lambda f: f.pad == 0),
    ('ld_out = H + 1', lambda f: f.pad == 1),
    ('ld_out = H rounded up to 32', lambda f: f.ld_out % 32 == 0 and f.pad > 1),
    ('rows * ld_out > 8192 * 256: grid-stride', lambda f: f.passes > 1),
    ('p = 0 without a mask: a padded copy', lambda f: f.kind == 'copy' and f.p == 0.0 and f.pad > 0),
    ('the backward call: src = dW with a longer row, ld_out = H', lambda f: f.backward and f.kind == 'hash'),
] + [('hash, p = %g' % p, (lambda p: lambda f: f.kind == 'hash' and f.p == p)(p)) for p in WD_P])
WD_CASES = [
    WDCase('mask-H', 37, 50, 53, 'H', 'mask', 0.0, 0, ['explicit mask', 'ld_src > H', 'ld_out = H']),
    WDCase('mask-H1', 37, 50, 50, 'H+1', 'mask', 0.0, 0, ['explicit mask', 'ld_out = H + 1']),
    WDCase('mask-32', 37, 50, 53, 'ceil32', 'mask', 0.0, 0, ['explicit mask', 'ld_out = H rounded up to 32']),
    WDCase('copy', 9, 1150, 1150, 'ceil32', 'copy', 0.0, 5, ['p = 0 without a mask: a padded copy']),
    WDCase('hash-.25', 37, 50, 53, 'ceil32', 'hash', 0.25, WD_SEEDS[1], ['hash, p = 0.25']),
    WDCase('hash-.5', 64, 115, 115, 'H+1', 'hash', 0.5, WD_SEEDS[2], ['hash, p = 0.5']),
    WDCase('hash-.9', 37, 50, 50, 'H', 'hash', 0.9, WD_SEEDS[3], ['hash, p = 0.9']),
    WDCase('bwd', 64, 115, 116, 'H', 'hash', 0.5, WD_SEEDS[2], ['the backward call: src = dW with a longer row, ld_out = H']),
    WDCase('big', 1100, 1900, 1900, 'ceil32', 'hash', 0.25, WD_SEEDS[0], ['rows * ld_out > 8192 * 256: grid-stride']),
]


def wd_keep(seed, idx, p):
    "wd_keep of csrc/text.hip in numpy: keep[i] = [u >= p], u = the top 24 bits of splitmix64(seed + idx * golden) / 2^24"
    with np.errstate(over='ignore'):
        x = np.uint64(seed) + np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    u = (x >> np.uint64(40)).astype(np.float64) / 16777216.0               # 24 bits: exact in fp32 as well
    return u >= np.float64(F32(p))


def wd_scale(p):
    return F32(1.0) / (F32(1.0) - F32(p))


def wd_data(c):
    r = np.random.RandomState(c.rows + c.H)
    assert c.rows * max(c.ld_src, wd_ld_out(c.H, c.ld_out)) <= MAX_ELEMS
    src = r.randn(c.rows, c.ld_src).astype(F32)
    mask = None
    if c.kind == 'mask':
        mask = (r.choice([0.0, 2.0, 1.0 / 0.7], (c.rows, c.H))).astype(F32)
    return src, mask


def wd_reference(c, src, mask, index_by_ld_out=False):
    "fp32 out [rows, ld_out] (bit for bit) and the keep pattern; index_by_ld_out builds the mutant that hashes r * ld_out + c"
    ld_out = wd_ld_out(c.H, c.ld_out)
    rr, cc = np.meshgrid(np.arange(c.rows), np.arange(c.H), indexing='ij')
    keep = None
    if c.kind == 'mask':
        m = mask.astype(np.float64)
    elif c.kind == 'hash' and c.p > 0:
        keep = wd_keep(c.seed, rr * (ld_out if index_by_ld_out else c.H) + cc, c.p)
        m = np.where(keep, np.float64(wd_scale(c.p)), 0.0)
    else:
        m = np.ones((c.rows, c.H))
    out = np.zeros((c.rows, ld_out), dtype=F32)
    out[:, :c.H] = (src[:, :c.H].astype(np.float64) * m).astype(F32)
    return out, keep


def check_wd(c, src, mask, got, ctx=''):
    want, keep = wd_reference(c, src, mask)
    got = np.asarray(got, dtype=F32)
    assert not got[:, c.H:].any() and not np.signbit(got[:, c.H:]).any(), '%s: a pad column is not +0' % ctx
    if keep is not None:
        nz = src[:, :c.H] != 0
        assert np.array_equal((got[:, :c.H] != 0)[nz], keep[nz]), '%s: the keep pattern differs from the restated hash' % ctx
    _same_bits(got, want, 'out', ctx)                                       # (a dropped negative is -0 in both)
    return keep


def wd_share_sigmas(keep, p):
    "how many standard deviations of binomial(n, 1 - p) the kept count lies from its mean"
    n = keep.size
    return abs(float(keep.sum()) - n * (1 - p)) / np.sqrt(n * p * (1 - p))


def fmt_ratios(r):
    return '  '.join('%s %.3f' % kv for kv in r.items())


if __name__ == '__main__':
    for c in CE_CASES:
        print('ce', c.name, ce_facts(c))
    for c in EMB_CASES:
        print('emb', c.name, emb_facts(c))
    for c in REG_CASES:
        print('reg', c.name, reg_facts(c))
    for c in WD_CASES:
        print('wd', c.name, wd_facts(c))
