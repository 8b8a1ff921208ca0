"""The case tables of the tabular / collab embedding C-ABI sweep (tests/test_embed_abi_gpu.py, tests/test_embed_cases_cpu.py) and their
fp64 references.

A plain module: no fixtures, nothing from the library.  It covers csrc/tabular.hip (nnl_tab_renorm, nnl_tab_gather_fwd,
nnl_tab_scatter_bwd, nnl_tab_scan_bwd, nnl_pad_cols, nnl_keep_masks), csrc/embdotbias.hip (nnl_embdotbias_fwd / _bwd) and
csrc/linear_small.hip (nnl_linear_small_fwd / _bwd).  Every case exists for a regime of a kernel's loops or of the route selection and
names it; the *_facts() functions derive the regime from the sizes and the index vectors alone, the *_REGIMES tables hold the predicates,
and the CPU test checks every claim and that no regime is left without a case.  U = 2^-24.

Everything that sums runs in two data modes.  `int`: small integers (values in [-4, 4], masks in {0, 1, 2}), every partial sum exact
below 2^24 (asserted), compared BIT FOR BIT on every route, the atomic one included.  `randn`: the bounds below, counted from the
kernels' own operations (the library is built with -ffp-contract=off: a product and a sum round separately).

tab_gather_fwd  out = fl(W[x] * row_mask) / fl(cont * cont_mask): one product, bit for bit in every mode; an index outside [0, card)
                (-1, card, 2^32 + 1) gives zero columns; pad columns are +0.
tab_renorm      a row whose fp32 norm is not above max_norm (strict >) and a row nobody looks up keep their bits.  A scaled row:
                relative U ((A + 5) / 2 + 5), A = ceil(d / 16) + 4 additions on the way of a square into ss (lane steps and the four
                levels of the 16-lane tree) and the square itself 1U: (A + 1) U on ss, half of it on the root; then sqrtf 1U, + 1e-7f 1U,
                the division 1U, the product 1U, +1.  All other rows stay a relative 2^-12 away from max_norm (asserted on the fp64
                norms: a condition on the inputs), so that the branch taken is that of the reference.
tab_*_bwd       dtab: U (len + 2) sum |term| per element, term = dout * row_mask (one product, 1U; at most len additions on any of
                the three routes: in sample order in the scan, SL slots and a tree in the sorted scatter, any order with atomics), +1.
                dcont = fl(dout * cont_mask): bit for bit.  A sample with an index outside [0, card) adds nothing; rows nobody
                looked up are +0.
embdotbias_fwd  z: U (ceil(D / 16) + 4 + 2 + 1) (sum |u m| + |bu| + |bi|): the fmaf steps of a lane, four tree levels, two bias
                additions, +1.  y = lo + (hi - lo) sigmoid(z): (hi - lo) s (1 - s) times the bound of z (the slope of the sigmoid), plus
                U (6 (hi - lo) s + |y|): expf 2U, 1 + e, the division and the product with (hi - lo) 1U each, +1; the last addition
                U |y|.  hi - lo is formed in fp32 by the reference as well.
embdotbias_bwd  z is an INPUT (fp32 values, the same in the reference), so the bound is that of the pass alone.  With e = expf(-z)
                (2U) and s = 1 / (1 + e) (two roundings) the computed s is off by at most 4U s; 1 - s then carries the ABSOLUTE error
                4U s (+ U (1 - s) where s < 1/2; the subtraction is exact above), not a relative one.  Three products (hi - lo) * s,
                * (1 - s), dy *: 3U; the error of s in the factor s: 4U; +1:
                  g:  U |dy| (hi - lo) (9 s (1 - s) + 4 s) + 2^-126 |dy| (hi - lo)
                — the `4 s` term is what keeps saturated samples in range: at z = 30 fp32 has s = 1, 1 - s = 0 and g = 0 against
                9.4e-14 |dy| (hi - lo); the last term lets a g below the normal range come out as 0 (z = -100: expf overflows, s = 0).
                dU[u, d] = sum g m: sum (g bound) |m| + U (len + 2) sum |g m| (the product 1U, at most len additions, +1); dM alike;
                dbu / dbi: sum (g bound) + U (len + 2) sum |g|.  Without a range g = dy exactly.  A sample with ONE index out of
                range is skipped and its partner row never read (the tables sit in a NaN arena).
linear_small    forward: U (ceil(K / 64) + 6 + 1 + 1) (sum |x w| + |bias|): lane steps, six tree levels, the bias, the product.
                dw / db: U (16 + 3 + nslab + 1) sum |dy x| (16 rows of a group in order, three additions across the groups, the slabs in
                order, the product).  dx: U (N + 1) sum |dy w|.  `int` mode bit for bit.
pad_cols, keep_masks   bit for bit; keep_masks gives exactly fl(1 / keep) where u < keep (strictly) and +0 elsewhere.

Measured on an MI355X, max err / bound over the sweep (tests/test_embed_abi_gpu.py prints them per case):
  tab_gather, pad_cols, keep_masks, dcont    bit for bit in every case and mode
  tab_*_bwd     int    bit for bit on the scan, the sorted and the atomic route (three ways into it, and bs = 32769)
                randn  dtab 0.406 on each of the three routes (the longest segments are 65 samples: the routes' orders hardly differ);
                       bs = 32769 with rows of 3600 .. 16000 samples below 0.0005: the bound grows with len, the error with its root
  tab_renorm    scaled rows 0.307; rows below or at max_norm and rows nobody looked up bit for bit; flags zero, err_flag as the reference's
  embdotbias    int    z, dU, dM, dbu, dbi bit for bit on all five routes; y (with a range, so not exact) 0.942: at z << 0 y = 0.5 + tiny
                       and the half ulp of the last addition is the whole U |y|
                randn  route                 z      y      dU     dM     dbu    dbi
                       scan                  0.139  0.219  0.264  0.225  0.220  0.204
                       det:one_block         0.228  0.403  0.259  0.320  0.252  0.177
                       det:four_fills        0.132  0.176  0.308  0.249  0.306  0.101
                       atomic:one_block      0.261  0.403  0.207  0.174  0.215  0.059
                       atomic:four_fills     0.041  0.048  0.123  0.146  0.087  0.068   (one case, n = 17)
                       saturated samples (z = +-30, +-100, +-17, ...) are inside these figures, none excused
  linear_small  int    bit for bit;  randn  y 0.146  dx 0.604  dw 0.098  db 0.054 (dw / db: ~20 + nslab additions counted one after the
                       other on sums of up to 1025 products whose roundings average out; M = 1 .. 5, where they cannot, give the maxima)
  fp32 numpy restatements of the summation orders (tests/test_embed_cases_cpu.py) against the same bounds: dtab 0.41, z 0.23, y 0.40,
  dU 0.31, dM 0.32, renorm 0.31, linear y 0.15 dx 0.60 dw 0.11
  The library before this sweep: the scan backward failed every case with an index 2^32 + r whose sample carried a gradient (it narrowed
  to int before the range check and credited row r); nnl_linear_small_bwd left dw / db unwritten at M = 0 and wrote dx before refusing a
  short workspace.
"""
import collections

import numpy as np

from optim_cases import U, _ratio, _same_bits, cdiv

F32 = np.float32
TWO32 = 2 ** 32
TINY = 2.0 ** -126
DET_MAX = 32768                                  # nnl_det::kMaxSamples: above it the sorted scatter is not taken
MODES = ('int', 'randn')


def case_id(c):
    return c.name


def dl_sl(D):
    "scatter_det.h: DL = the power of two >= min(D, 64) element lanes, SL = 64 / DL sample slots"
    DL = 1
    while DL < D and DL < 64:
        DL <<= 1
    return DL, 64 // DL


def plan_indices(card, dim, n, seed, invalid):
    """int64 indices [n] into a table of `card` rows (text_cases.emb_indices per column, SL from the column's dim): row 0 once, row 1 SL
    times, row 2 SL + 1 times, row 3 64 times, row 4 65 times (as far as card and n allow), the top row card - 1 1 + 64 k times, the rest
    random over the rows in between; all at shuffled positions.  invalid: three of the random ones become -1, card and 2^32 + 1 (or
    2^32 + 0 in a one-row table)."""
    r = np.random.RandomState(seed * 7919 + card * 31 + dim * 3 + n)
    _, SL = dl_sl(dim)
    x, left = [], n
    k = max((n // 3 - 1) // 64, 0)
    plan = [(card - 1, 1 + 64 * k if n >= 3 else 0), (0, 1), (1, SL), (2, SL + 1), (3, 64), (4, 65)]
    for i, (row, cnt) in enumerate(plan):
        if 0 < cnt <= left and 0 <= row < card and (i == 0 or row < card - 1):
            x += [row] * cnt
            left -= cnt
    if left:
        lo, hi = (5, card - 1) if card > 7 else (0, card)
        x += r.randint(lo, hi, left).tolist()
    x = np.asarray(x, dtype=np.int64)
    if invalid and left >= 3:
        alias = TWO32 + min(1, card - 1)
        x[n - 1], x[n - 2], x[n - 3] = -1, card, alias
    return x[r.permutation(n)] if n else x


def seg_facts(x, card, dim):
    "(sorted set of segment lengths, SL, length of the top row's segment if it ends the sorted array else 0)"
    _, SL = dl_sl(dim)
    ok = (x >= 0) & (x < card)
    cnt = np.bincount(x[ok], minlength=card) if ok.any() else np.zeros(card, dtype=np.int64)
    top = int(x.max()) if x.size else -1
    return sorted(set(int(c) for c in cnt if c > 0)), SL, (int(cnt[top]) if 0 <= top < card else 0)


SEG_REGIMES = [
    ('segment of length 1', lambda f: any(1 in l for l, _, _ in f.segs)),
    ('segment of 2 .. SL samples', lambda f: any(any(1 < v <= sl for v in l) for l, sl, _ in f.segs)),
    ('segment of SL + 1 samples', lambda f: any(sl + 1 in l for l, sl, _ in f.segs)),
    ('segment of 64 samples', lambda f: any(64 in l for l, _, _ in f.segs)),
    ('segment of 65 samples: a second ballot round', lambda f: any(65 in l for l, _, _ in f.segs)),
    ('last segment ends the sorted array after 1 + 64 k positions', lambda f: any(e > 1 and e % 64 == 1 for _, _, e in f.segs)),
]
_S1, _SS, _SG, _S64, _S65, _LAST = (n for n, _ in SEG_REGIMES)


# ======================================================================================================================================
# the tabular front end: gather, the three backward routes
# ======================================================================================================================================
TAB_GRID = 4096 * 256                            # threads of grid_for()'s largest grid in tabular.hip
SCAN_MAX_DIM = 32                                # kScanMaxDim
TabCase = collections.namedtuple('TabCase', 'name bs cards dims n_cont pad row_mask cont_mask dcont invalid regimes')
TabFacts = collections.namedtuple('TabFacts', 'bs ncat dims sizes n_cont pad row_mask cont_mask dcont invalid passes segs stages ragged '
                                              'cont_tail by_size')


def tab_layout(case):
    "col_off, row_off, grad_off, col_table, row_table, blk_col, blk_first, cat_width, total_rows, grad_elems (ops.TabularPlan restated)"
    dims, cards = list(case.dims), list(case.cards)
    sizes = [c * d for c, d in zip(cards, dims)]
    z = lambda a: np.concatenate([[0], np.cumsum(a)[:-1]]) if len(a) else np.zeros(0)
    blk_col, blk_first = [], []
    for j, n in enumerate(sizes):
        for f in range(0, n, 256):
            blk_col.append(j)
            blk_first.append(f)
    return dict(col_off=z(dims).astype(np.int32), row_off=z(cards).astype(np.int32), grad_off=z(sizes).astype(np.int64),
                col_table=np.repeat(np.arange(len(dims)), dims).astype(np.int32), row_table=np.repeat(np.arange(len(cards)), cards).astype(np.int32),
                blk_col=np.asarray(blk_col or [0], dtype=np.int32), blk_first=np.asarray(blk_first or [0], dtype=np.int32), n_scan=len(blk_col),
                cat_width=int(sum(dims)), total_rows=int(sum(cards)), grad_elems=int(sum(sizes)), card=np.asarray(cards, dtype=np.int32),
                dim=np.asarray(dims, dtype=np.int32))


def tab_xcat(case):
    "[bs, ncat]; the invalid indices go into the odd columns (and into the only column), so that an even column's top row ends the sort"
    ncat = len(case.cards)
    cols = [plan_indices(case.cards[j], case.dims[j], case.bs, j + 1, case.invalid and (j % 2 == 1 or ncat == 1)) for j in range(ncat)]
    return np.stack(cols, axis=1) if ncat else np.zeros((case.bs, 0), dtype=np.int64)


def tab_facts(case):
    x = tab_xcat(case)
    ncat = len(case.cards)
    width = sum(case.dims) + case.n_cont
    segs = [seg_facts(x[:, j], case.cards[j], case.dims[j]) for j in range(ncat)]
    bad = bool(ncat and any((((x[:, j] < 0).any() and (x[:, j] == case.cards[j]).any() and (x[:, j] >= TWO32).any())) for j in range(ncat)))
    return TabFacts(case.bs, ncat, tuple(case.dims), tuple(c * d for c, d in zip(case.cards, case.dims)), case.n_cont, case.pad, case.row_mask,
                    case.cont_mask, case.dcont, bad, cdiv(case.bs * (width + case.pad), TAB_GRID), segs, cdiv(case.bs, 256), case.bs % 256,
                    (case.bs * case.n_cont) % 256, case.bs > DET_MAX)


GATHER_REGIMES = collections.OrderedDict(
    [('bs = %d' % b, (lambda b: lambda f: f.bs == b)(b)) for b in (0, 1, 255, 256, 257)] + [
        ('ncat = 0: continuous only', lambda f: f.ncat == 0 and f.n_cont > 0),
        ('n_cont = 0', lambda f: f.n_cont == 0 and f.ncat > 0),
        ('row_mask NULL', lambda f: not f.row_mask),
        ('row_mask with zeros', lambda f: f.row_mask and f.ncat > 0),
        ('cont_mask NULL', lambda f: not f.cont_mask and f.n_cont > 0),
        ('ld_out > cat_width + n_cont: pad columns', lambda f: f.pad > 0),
        ('dims 1, 3, 25 and 50 in one call', lambda f: set(f.dims) >= {1, 3, 25, 50}),
        ('one column', lambda f: f.ncat == 1),
        ('grid-stride: bs * ld_out > 4096 * 256', lambda f: f.passes > 1),
        ('indices -1, card and 2^32 + 1', lambda f: f.invalid),
    ])
_MIX = 'dims 1, 3, 25 and 50 in one call'
_PAD, _RM0, _RMN, _CMN, _BAD = ('ld_out > cat_width + n_cont: pad columns', 'row_mask with zeros', 'row_mask NULL', 'cont_mask NULL',
                                'indices -1, card and 2^32 + 1')
GATHER_CASES = [
    TabCase('bs0', 0, (5, 7), (3, 2), 2, 0, False, False, True, False, ['bs = 0', _RMN]),
    TabCase('bs1', 1, (5,), (3,), 0, 0, False, False, True, False, ['bs = 1', 'one column', 'n_cont = 0', _RMN]),
    TabCase('cont-only', 255, (), (), 7, 1, False, True, True, False, ['bs = 255', 'ncat = 0: continuous only', _PAD]),
    TabCase('mix256', 256, (9, 4, 30, 12), (1, 3, 25, 50), 5, 4, True, True, True, True, ['bs = 256', _MIX, _PAD, _RM0, _BAD]),
    TabCase('mix257', 257, (12, 30, 4, 9), (50, 25, 3, 1), 3, 0, True, False, True, True, ['bs = 257', _MIX, _RM0, _CMN, _BAD]),
    TabCase('one-col', 300, (40,), (25,), 0, 3, True, False, True, True, ['one column', 'n_cont = 0', _PAD, _BAD]),
    TabCase('stride', 4100, (9, 4, 30, 12), (1, 3, 25, 50), 170, 8, True, True, True, True, ['grid-stride: bs * ld_out > 4096 * 256', _MIX]),
]

BWD_DIMS = (1, 2, 3, 5, 7, 16, 25, 32)
BWD_REGIMES = collections.OrderedDict(
    [('dj = %d' % d, (lambda d: lambda f: d in f.dims)(d)) for d in BWD_DIMS] +
    [('bs = %d' % b, (lambda b: lambda f: f.bs == b)(b)) for b in (1, 255, 256, 257, 513)] + [
        ('a column of card * dim < 256: one partial block', lambda f: any(s < 256 for s in f.sizes)),
        ('a column of card * dim = 256', lambda f: 256 in f.sizes),
        ('a column of card * dim >= 257: several blocks, the last partial', lambda f: any(s > 256 and s % 256 for s in f.sizes)),
        ('the block table crosses from one column to the next', lambda f: f.ncat >= 2),
        ('ragged last 256-sample stage', lambda f: f.stages >= 2 and f.ragged > 0),
        ('row_mask NULL', lambda f: not f.row_mask),
        ('row_mask with zeros', lambda f: f.row_mask),
        ('n_cont = 0', lambda f: f.n_cont == 0),
        ('dcont NULL with n_cont > 0', lambda f: f.n_cont > 0 and not f.dcont),
        ('cont_mask NULL', lambda f: f.n_cont > 0 and f.dcont and not f.cont_mask),
        ('bs * n_cont not a multiple of 256', lambda f: f.dcont and f.cont_tail > 0),
        ('row-strided dout', lambda f: f.pad > 0),
        ('indices -1, card and 2^32 + r', lambda f: f.invalid),
        ('bs = 32769, two narrow columns: too many samples for the sort', lambda f: f.by_size and f.ncat == 2 and max(f.dims) <= 2),
    ] + SEG_REGIMES)
_X, _STR, _BADR = ('the block table crosses from one column to the next', 'row-strided dout', 'indices -1, card and 2^32 + r')
_LT, _EQ, _GT = ('a column of card * dim < 256: one partial block', 'a column of card * dim = 256',
                 'a column of card * dim >= 257: several blocks, the last partial')
BWD_CASES = [
    TabCase('bs1', 1, (5,), (3,), 0, 0, False, False, False, False, ['bs = 1', 'dj = 3', 'n_cont = 0', 'row_mask NULL', _S1, _LT]),
    TabCase('bs255', 255, (8, 128), (32, 2), 3, 0, True, False, False, True, ['bs = 255', 'dj = 32', 'dj = 2', _EQ, _X, 'row_mask with zeros',
                                                                            'dcont NULL with n_cont > 0', _BADR, _S1, _SS, _SG, _S64, _S65]),
    TabCase('bs256', 256, (7, 20), (5, 16), 3, 0, True, False, True, False, ['bs = 256', 'dj = 5', 'dj = 16', 'cont_mask NULL', _GT, _LT]),
    TabCase('bs257', 257, (40, 11), (7, 25), 2, 5, True, True, True, True, ['bs = 257', 'dj = 7', 'dj = 25', 'ragged last 256-sample stage', _STR,
                                                                          _BADR, _GT, _X, _LAST]),
    TabCase('bs513', 513, (300, 9, 50), (1, 3, 2), 5, 3, True, True, True, True, ['bs = 513', 'dj = 1', 'dj = 3', 'dj = 2', _S1, _SS, _SG, _S64,
                                                                                 _S65, _LAST, _BADR, _STR, 'ragged last 256-sample stage',
                                                                                 'bs * n_cont not a multiple of 256']),
    TabCase('narrow', 32769, (4, 6), (1, 2), 0, 0, True, False, False, True, ['bs = 32769, two narrow columns: too many samples for the sort',
                                                                            _BADR]),
]


def _vals(r, mode, shape):
    return (r.randint(-4, 5, shape) if mode == 'int' else r.randn(*shape)).astype(F32)


def _mask(r, mode, shape, keep):
    m = r.randint(0, 3, shape) if mode == 'int' else r.choice([0.0, 1.0 / keep], shape, p=[0.25, 0.75])
    return m.astype(F32)


def tab_data(case, mode):
    "xcat, tables, row_mask [ncat, bs], cont, cont_mask, dout [bs, width + pad] (the pad columns hold values nobody may read into a sum)"
    r = np.random.RandomState(len(case.name) * 101 + case.bs + (0 if mode == 'int' else 1000))
    L = tab_layout(case)
    ncat, bs, width = len(case.cards), case.bs, L['cat_width'] + case.n_cont
    x = tab_xcat(case)
    rm = _mask(r, mode, (ncat, bs), 0.9) if case.row_mask and ncat else None
    if rm is not None and bs:
        rm[:, 0] = 0                                                          # a zero in every column, and (int mode) a two
        rm[:, -1] = 2 if mode == 'int' else rm[:, -1]
    dout = _vals(r, mode, (bs, width + case.pad))
    for j in range(ncat):                                                     # a sample whose index would alias a row carries a gradient that shows
        for b in np.flatnonzero(x[:, j] >= TWO32):
            o = L['col_off'][j]
            dout[b, o:o + case.dims[j]] = np.where(dout[b, o:o + case.dims[j]] == 0, 1, dout[b, o:o + case.dims[j]])
            if rm is not None:
                rm[j, b] = 2 if mode == 'int' else F32(1.0 / 0.9)
    cont = _vals(r, mode, (bs, case.n_cont)) if case.n_cont else None
    cm = _mask(r, mode, (bs, case.n_cont), 0.8) if case.cont_mask and case.n_cont else None
    return dict(x=x, tables=[_vals(r, mode, (c, d)) for c, d in zip(case.cards, case.dims)], row_mask=rm, cont=cont, cont_mask=cm,
                dout=dout, L=L, mode=mode, case=case)


def tab_fwd_ref(d, pad_nonzero=False):
    "out [bs, ld_out] fp32, bit for bit (the fp64 product of two fp32 numbers rounded once is the fp32 product)"
    case, L = d['case'], d['L']
    bs, ncat = case.bs, len(case.cards)
    out = np.zeros((bs, L['cat_width'] + case.n_cont + case.pad))
    for j in range(ncat):
        idx = d['x'][:, j]
        ok = (idx >= 0) & (idx < case.cards[j])
        v = d['tables'][j].astype(np.float64)[np.where(ok, idx, 0)]
        if d['row_mask'] is not None:
            v = v * d['row_mask'][j].astype(np.float64)[:, None]
        out[:, L['col_off'][j]:L['col_off'][j] + case.dims[j]] = np.where(ok[:, None], v, 0.0)
    if case.n_cont:
        c = d['cont'].astype(np.float64)
        out[:, L['cat_width']:L['cat_width'] + case.n_cont] = c if d['cont_mask'] is None else c * d['cont_mask'].astype(np.float64)
    if pad_nonzero and case.pad:
        out[:, -1] = 1.0
    return out.astype(F32)


def check_tab_fwd(d, got, ctx=''):
    case, want = d['case'], tab_fwd_ref(d)
    got = np.asarray(got, dtype=F32).reshape(want.shape)
    if case.pad:
        assert not got[:, -case.pad:].any() and not np.signbit(got[:, -case.pad:]).any(), '%s: a pad column is not +0' % ctx
    _same_bits(got, want, 'out', ctx)


TAB_MUTANTS = ('drop_sample', 'drop_last_stage', 'mask_next_col', 'mask_transposed', 'col_off_shift', 'alias_2^32')


def tab_bwd_ref(d, mutant=None):
    """fp64 dtab (flat, grad_off order), its randn bound U (len + 2) sum |term|, and dcont fp32 (None when not asked for).  mutant: one of
    TAB_MUTANTS — the wrong kernels that the checker has to refuse."""
    case, L = d['case'], d['L']
    bs, ncat = case.bs, len(case.cards)
    dout = d['dout'].astype(np.float64)
    rm = d['row_mask']
    if rm is not None and mutant == 'mask_transposed':
        rm = rm.ravel()[(np.arange(bs)[None, :] * ncat + np.arange(ncat)[:, None]) % rm.size].reshape(ncat, bs)
    dtab, bound = np.zeros(L['grad_elems']), np.zeros(L['grad_elems'])
    dropped = False
    for j in range(ncat):
        idx, card, dj = d['x'][:, j].copy(), case.cards[j], case.dims[j]
        if mutant == 'alias_2^32':
            idx = np.where(idx >= TWO32, idx - TWO32, idx)
        use = (idx >= 0) & (idx < card)
        coff = L['col_off'][j] + (1 if mutant == 'col_off_shift' else 0)
        term = dout[:, coff:coff + dj]
        if rm is not None:
            term = term * rm[(j + 1) % ncat if mutant == 'mask_next_col' else j].astype(np.float64)[:, None]
        if mutant == 'drop_last_stage':
            use[256 * ((bs - 1) // 256):] = False
        if mutant == 'drop_sample' and not dropped:
            cnt = np.bincount(idx[use], minlength=card)
            for b in np.flatnonzero(use)[::-1]:
                if cnt[idx[b]] > 1 and term[b].all():
                    use[b], dropped = False, True
                    break
        g, a = np.zeros((card, dj)), np.zeros((card, dj))
        np.add.at(g, idx[use], term[use])
        np.add.at(a, idx[use], np.abs(term[use]))
        cnt = np.bincount(idx[use], minlength=card).astype(np.float64)
        o = int(L['grad_off'][j])
        dtab[o:o + card * dj] = g.ravel()
        bound[o:o + card * dj] = (U * (cnt[:, None] + 2) * a).ravel()
    if mutant == 'drop_sample':
        assert dropped, 'no row with two samples and a non-zero term'
    dcont = None
    if case.n_cont and case.dcont:
        g = dout[:, L['cat_width']:L['cat_width'] + case.n_cont]
        dcont = (g if d['cont_mask'] is None else g * d['cont_mask'].astype(np.float64)).astype(F32)
    return dtab, bound, dcont


def tab_int_is_exact(d):
    "every partial sum of the int data is an integer below 2^24: sum |term| bounds them all"
    case, L = d['case'], d['L']
    m = 1.0 if d['row_mask'] is None else float(np.abs(d['row_mask']).max(initial=0))
    worst = float(np.abs(d['dout']).max(initial=0)) * m * case.bs
    return d['mode'] == 'int' and worst < 2 ** 24 and all(np.array_equal(v, np.round(v)) for v in [d['dout']] + d['tables'])


def check_tab_bwd(d, dtab, dcont, ctx=''):
    "ratio max err / bound of dtab (0.0 in int mode: bit for bit); dcont bit for bit"
    want, bound, want_c = tab_bwd_ref(d)
    dtab = np.asarray(dtab, dtype=F32).ravel()[:want.size]
    if want_c is not None:
        _same_bits(np.asarray(dcont, dtype=F32).reshape(want_c.shape), want_c, 'dcont', ctx)
    assert not dtab[bound == 0].any() and not np.signbit(dtab[bound == 0]).any(), '%s: a table row without a gradient is not +0' % ctx
    if d['mode'] == 'int':
        assert tab_int_is_exact(d)
        _same_bits(dtab, want.astype(F32), 'dtab', ctx)
        return 0.0
    return _ratio(dtab, want, bound, 'dtab', ctx)


def scan_magic(dj):
    "the multiplier of tab_scan_bwd_kernel: ceil(2^32 / dj) (0 for dj = 1, which does not divide)"
    return (0x100000000 + dj - 1) // dj if dj > 1 else 0


# ======================================================================================================================================
# max_norm renormalisation
# ======================================================================================================================================
RENORM_DIMS = (1, 15, 16, 17, 25, 50)
MAX_NORM = 1.5
EPS7 = float(F32(1e-7))
RenormCase = collections.namedtuple('RenormCase', 'name bs cards dims invalid regimes')
RenormFacts = collections.namedtuple('RenormFacts', 'bs dims total_rows kinds max_lookups invalid untouched')
# rows of every table, by number: 0 below max_norm, 1 above, 2 exactly max_norm, 3 above and looked up by many samples, 4 .. card - 2
# random (half below, half above), card - 1 above and NEVER looked up


def renorm_xcat(case):
    r = np.random.RandomState(case.bs + len(case.cards))
    cols = []
    for j, card in enumerate(case.cards):
        x = r.randint(0, card - 1, case.bs)
        if case.bs >= 8:
            x[:3] = (0, 1, 2)
            x[3:8] = 3
        if case.invalid and case.bs >= 12:
            x[8:11] = (-1, card, TWO32 + 1)
        cols.append(x[r.permutation(case.bs)] if case.bs else x)
    return np.stack(cols, axis=1).astype(np.int64)


def renorm_data(case):
    r = np.random.RandomState(17 + case.bs)
    tables = []
    for card, d in zip(case.cards, case.dims):
        assert card >= 6
        w = r.randn(card, d)
        target = np.where(r.rand(card) < 0.5, 0.4 + 0.8 * r.rand(card), 2.0 + 2.0 * r.rand(card))
        target[[0, 1, 3, card - 1]] = (1.0, 3.0, 2.5, 3.5)
        w *= (target / np.sqrt((w * w).sum(axis=1)))[:, None]
        w[2] = 0
        if d >= 9:                                                             # nine entries of 0.5 spread over the lanes and passes:
            w[2, np.unique(np.linspace(0, d - 1, 9).round().astype(int))[:9]] = 0.5   # squares and partial sums exact, norm = 1.5
            assert (w[2] != 0).sum() == 9
        else:
            w[2, d - 1] = 1.5
        tables.append(w.astype(F32))
    return dict(x=renorm_xcat(case), tables=tables, case=case)


def renorm_facts(case):
    d = renorm_data(case)
    kinds, looks, untouched = set(), 0, False
    for j, (card, w) in enumerate(zip(case.cards, d['tables'])):
        idx = d['x'][:, j]
        ok = (idx >= 0) & (idx < card)
        cnt = np.bincount(idx[ok], minlength=card)
        norm = np.sqrt((w.astype(np.float64) ** 2).sum(axis=1))
        for row in np.flatnonzero(cnt):
            kinds.add('equal' if norm[row] == MAX_NORM else 'below' if norm[row] < MAX_NORM else 'above')
        looks = max(looks, int(cnt.max(initial=0)))
        untouched |= bool(((cnt == 0) & (norm > MAX_NORM)).any())
    bad = bool(any((d['x'][:, j] < 0).any() and (d['x'][:, j] >= case.cards[j]).any() for j in range(len(case.cards))))
    return RenormFacts(case.bs, tuple(case.dims), int(sum(case.cards)), kinds, looks, bad, untouched)


RENORM_REGIMES = collections.OrderedDict(
    [('d = %d' % d, (lambda d: lambda f: d in f.dims)(d)) for d in RENORM_DIMS] + [
        ('a row below max_norm', lambda f: 'below' in f.kinds),
        ('a row above max_norm', lambda f: 'above' in f.kinds),
        ('a row whose norm equals max_norm', lambda f: 'equal' in f.kinds),
        ('a row looked up by several samples', lambda f: f.max_lookups >= 5),
        ('rows above max_norm that nobody looks up', lambda f: f.untouched),
        ('total_rows * 16 not a multiple of 256', lambda f: f.total_rows % 16 != 0),
        ('total_rows * 16 a multiple of 256', lambda f: f.total_rows % 16 == 0),
        ('an out-of-range index sets the flag', lambda f: f.invalid),
        ('all indices valid: the flag stays 0', lambda f: not f.invalid and f.bs > 0),
        ('bs = 0', lambda f: f.bs == 0),
    ])
_RB, _RA, _RE, _RMANY, _RUN = ('a row below max_norm', 'a row above max_norm', 'a row whose norm equals max_norm',
                               'a row looked up by several samples', 'rows above max_norm that nobody looks up')
RENORM_CASES = [
    RenormCase('bs0', 0, (6, 7), (15, 16), False, ['bs = 0']),
    RenormCase('narrow', 40, (9, 8, 12), (1, 15, 16), False, ['d = 1', 'd = 15', 'd = 16', _RB, _RA, _RE, _RMANY, _RUN,
                                                             'total_rows * 16 not a multiple of 256', 'all indices valid: the flag stays 0']),
    RenormCase('wide', 300, (10, 11, 11), (17, 25, 50), True, ['d = 17', 'd = 25', 'd = 50', _RB, _RA, _RE, _RMANY, _RUN,
                                                              'total_rows * 16 a multiple of 256', 'an out-of-range index sets the flag']),
]


def renorm_ref(d, mutant=None):
    """per table: the fp64 result, the bound (0 = bit for bit), and the looked-up mask; the flag.  mutant 'untouched': every row is
    renormed; 'ge': the comparison is >= (the exact row is scaled by 1.5 / (1.5 + 1e-7))"""
    case = d['case']
    out, flag = [], 0
    for j, (card, dj, w) in enumerate(zip(case.cards, case.dims, d['tables'])):
        idx = d['x'][:, j]
        ok = (idx >= 0) & (idx < card)
        flag |= int((~ok).any())
        hit = np.bincount(idx[ok], minlength=card) > 0
        w64 = w.astype(np.float64)
        norm = np.sqrt((w64 * w64).sum(axis=1))
        assert (np.abs(norm[norm != MAX_NORM] - MAX_NORM) >= 2.0 ** -12 * MAX_NORM).all(), 'a norm too close to max_norm'
        scaled = (hit | (mutant == 'untouched')) & ((norm >= MAX_NORM) if mutant == 'ge' else (norm > MAX_NORM))
        want = np.where(scaled[:, None], w64 * (MAX_NORM / (norm + EPS7))[:, None], w64)
        bound = np.where(scaled[:, None], U * ((cdiv(dj, 16) + 4 + 1) / 2.0 + 5) * np.abs(want), 0.0)
        out.append((want, bound))
    return out, flag


def check_renorm(d, tables, flag, flags_after, ctx=''):
    want, want_flag = renorm_ref(d)
    assert int(flag) == want_flag, '%s: err_flag %r, want %d' % (ctx, flag, want_flag)
    assert not np.asarray(flags_after).any(), '%s: the row flags are not all zero on exit' % ctx
    worst = 0.0
    for j, ((w, bound), got) in enumerate(zip(want, tables)):
        got = np.asarray(got, dtype=F32).reshape(w.shape)
        keep = (bound == 0).all(axis=1)
        _same_bits(got[keep], d['tables'][j][keep], 'table %d: rows that keep their bits' % j, ctx)
        worst = max(worst, _ratio(got[~keep].ravel(), w[~keep].ravel(), bound[~keep].ravel(), 'table %d: scaled rows' % j, ctx))
    return worst


# ======================================================================================================================================
# EmbeddingDotBias
# ======================================================================================================================================
ED_FWD_GRID = 2048 * 16                          # samples of the forward's largest grid
ED_SCAN_MAX_N = 256
ED_SCAN_MAX_PAIRS = 1 << 27
ED_LO, ED_HI = 0.5, 4.5                          # hi - lo = 4: exact, and 4 * 0.5 * 0.5 = 1 keeps the int mode exact at z = 0
EDCase = collections.namedtuple('EDCase', 'name n n_user n_item D has_range layout ws env zmode invalid err_flag regimes')
EDFacts = collections.namedtuple('EDFacts', 'n D has_range route fwd_passes zmode half_bad err_flag pairs segs_u segs_i z_out env')


def ed_route(case):
    "the route note nnl_embdotbias_bwd has to leave (None: nothing is launched but the fills)"
    env = case.env or {}
    adjacent = case.layout == 'block'
    tot = (case.n_user + case.n_item) * (case.D + 1)
    if (adjacent and 1 <= case.n <= ED_SCAN_MAX_N and tot < 2 ** 31 and tot * case.n <= ED_SCAN_MAX_PAIRS
            and env.get('NNL_EMBDOT_SCAN', '1') != '0' and env.get('NNL_SCATTER_ATOMIC', '0') == '0'):
        return 'embdot_bwd<scan>'
    if case.n == 0:
        return None
    fills = ':one_block' if adjacent else ':four_fills'
    det = case.ws == 'full' and case.n <= DET_MAX and env.get('NNL_SCATTER_ATOMIC', '0') == '0'
    return ('embdot_bwd<det>' if det else 'embdot_bwd<atomic>') + fills


def ed_x(case):
    "[n, 2]: both columns by plan_indices; invalid: samples with a bad item and a good user and the reverse, never both bad"
    u = plan_indices(case.n_user, case.D, case.n, 11, False)
    it = plan_indices(case.n_item, 1, case.n, 12, False)
    x = np.stack([u, it], axis=1) if case.n else np.zeros((0, 2), dtype=np.int64)
    if case.invalid:
        assert case.n >= 16
        r = np.random.RandomState(case.n)
        free = np.flatnonzero((u >= 5) & (u < case.n_user - 1) & (it >= 5) & (it < case.n_item - 1))      # leave the planned segments whole
        pool = free if free.size >= 6 else np.arange(case.n)
        pos = pool[r.permutation(pool.size)[:6]]
        x[pos[:3], 1] = (-1, case.n_item, TWO32 + 1)
        x[pos[3:], 0] = (-1, case.n_user, TWO32 + 1)
    return x


def ed_facts(case):
    x = ed_x(case)
    ok_u, ok_i = (x[:, 0] >= 0) & (x[:, 0] < case.n_user), (x[:, 1] >= 0) & (x[:, 1] < case.n_item)
    return EDFacts(case.n, case.D, case.has_range, ed_route(case), cdiv(case.n, ED_FWD_GRID), case.zmode, bool((ok_u ^ ok_i).any()),
                   case.err_flag, (case.n_user + case.n_item) * (case.D + 1) * case.n, [seg_facts(x[:, 0], case.n_user, case.D)],
                   [seg_facts(x[:, 1], case.n_item, case.D), seg_facts(x[:, 1], case.n_item, 1)], case.zmode != 'none', case.env or {})


def _seg(pred, which):
    return lambda f: pred(collections.namedtuple('S', 'segs')(getattr(f, which)))


ED_REGIMES = collections.OrderedDict(
    [('D = %d' % D, (lambda D: lambda f: f.D == D)(D)) for D in (1, 15, 16, 17, 30, 50, 128)] +
    [('n = %d' % n, (lambda n: lambda f: f.n == n)(n)) for n in (0, 1, 15, 16, 17, 256, 257)] + [
        ('forward grid-stride: n > 2048 * 16, D = 1', lambda f: f.fwd_passes > 1 and f.D == 1),
        ('has_range = 0', lambda f: not f.has_range),
        ('has_range = 1', lambda f: f.has_range),
        ('z NULL in the forward', lambda f: not f.z_out),
        ('err_flag NULL', lambda f: not f.err_flag),
        ('saturated z: |z| up to 30, and +-100', lambda f: f.zmode == 'saturated' and f.has_range),
        ('samples with one bad index', lambda f: f.half_bad),
        ('route scan', lambda f: f.route == 'embdot_bwd<scan>'),
        ('route det, one fill', lambda f: f.route == 'embdot_bwd<det>:one_block'),
        ('route det, four fills', lambda f: f.route == 'embdot_bwd<det>:four_fills'),
        ('route atomic, one fill', lambda f: f.route == 'embdot_bwd<atomic>:one_block'),
        ('route atomic, four fills', lambda f: f.route == 'embdot_bwd<atomic>:four_fills'),
        ('n = 256 adjacent: scan', lambda f: f.n == 256 and f.route == 'embdot_bwd<scan>'),
        ('n = 257 adjacent: det', lambda f: f.n == 257 and f.route == 'embdot_bwd<det>:one_block'),
        ('table elements x samples = 2^27: scan', lambda f: f.pairs == ED_SCAN_MAX_PAIRS and f.route == 'embdot_bwd<scan>'),
        ('table elements x samples just above 2^27: det', lambda f: ED_SCAN_MAX_PAIRS < f.pairs <= ED_SCAN_MAX_PAIRS + 2 * 256
         and f.route == 'embdot_bwd<det>:one_block'),
        ('NNL_EMBDOT_SCAN=0', lambda f: f.env.get('NNL_EMBDOT_SCAN') == '0' and f.n <= 256 and f.route == 'embdot_bwd<det>:one_block'),
        ('NNL_SCATTER_ATOMIC=1', lambda f: f.env.get('NNL_SCATTER_ATOMIC') == '1' and 'atomic' in (f.route or '')),
        ('n > 32768: too many samples for the sort', lambda f: f.n > DET_MAX and 'atomic' in f.route),
    ] + [('users: ' + n, _seg(p, 'segs_u')) for n, p in SEG_REGIMES] + [('items: ' + n, _seg(p, 'segs_i')) for n, p in SEG_REGIMES])
_SAT, _HB = 'saturated z: |z| up to 30, and +-100', 'samples with one bad index'
_R0, _R1 = 'has_range = 0', 'has_range = 1'
_EU = ['users: ' + n for n, _ in SEG_REGIMES]
_EI = ['items: ' + n for n, _ in SEG_REGIMES]
ED_CASES = [
    EDCase('n0', 0, 5, 6, 15, 1, 'block', 'full', None, 'normal', False, True, ['n = 0', 'D = 15', _R1]),
    EDCase('n1', 1, 5, 6, 16, 0, 'block', 'full', None, 'normal', False, True, ['n = 1', 'D = 16', _R0, 'route scan', _EU[0], _EI[0]]),
    EDCase('n15', 15, 5, 6, 17, 1, 'separate', 'full', None, 'none', False, False, ['n = 15', 'D = 17', 'route det, four fills',
                                                                                   'z NULL in the forward', 'err_flag NULL']),
    EDCase('n16', 16, 7, 6, 30, 1, 'block', 'full', None, 'saturated', True, True, ['n = 16', 'D = 30', _SAT, _HB, 'route scan']),
    EDCase('n17', 17, 7, 6, 50, 1, 'separate', 'null', None, 'normal', True, True, ['n = 17', 'D = 50', 'route atomic, four fills', _HB]),
    EDCase('n256', 256, 9, 300, 128, 1, 'block', 'full', None, 'saturated', True, True, ['n = 256', 'D = 128', 'n = 256 adjacent: scan', _SAT,
                                                                                         _HB] + _EI[:5]),
    EDCase('n257', 257, 300, 9, 1, 1, 'block', 'full', None, 'saturated', True, True, ['n = 257', 'D = 1', 'n = 257 adjacent: det',
                                                                                       'route det, one fill', _SAT, _HB] + _EU[:5]),
    EDCase('d3-600', 600, 40, 300, 3, 0, 'block', 'full', None, 'normal', True, True, [_R0, _HB] + _EU[:5] + _EI[:5]),
    EDCase('d30-600', 600, 300, 40, 30, 1, 'separate', 'full', None, 'saturated', True, True, ['D = 30', 'route det, four fills', _SAT, _HB] + _EU[:5]),
    EDCase('noscan', 64, 20, 30, 30, 1, 'block', 'full', {'NNL_EMBDOT_SCAN': '0'}, 'normal', True, True, ['NNL_EMBDOT_SCAN=0']),
    EDCase('env-atomic', 64, 20, 30, 30, 1, 'block', 'full', {'NNL_SCATTER_ATOMIC': '1'}, 'normal', True, True,
           ['NNL_SCATTER_ATOMIC=1', 'route atomic, one fill']),
    EDCase('pairs-2^27', 256, 262100, 44, 1, 1, 'block', 'full', None, 'normal', False, True, ['table elements x samples = 2^27: scan', _EU[5], _EI[5]]),
    EDCase('pairs-above', 256, 262100, 45, 1, 1, 'block', 'full', None, 'normal', False, True,
           ['table elements x samples just above 2^27: det']),
    EDCase('big', 40000, 50, 60, 1, 1, 'block', 'full', None, 'normal', True, True, ['forward grid-stride: n > 2048 * 16, D = 1',
                                                                                   'n > 32768: too many samples for the sort']),
]


def ed_data(case, mode):
    """x, U, M, bu, bi (fp32), z (the INPUT of the backward: fp32 values; int mode 0 with a range), dy.  int mode: g = dy exactly
    (no range, or (hi - lo) s (1 - s) = 4 * 1/2 * 1/2 at z = 0)."""
    r = np.random.RandomState(case.n + case.D + (0 if mode == 'int' else 1000))
    n, D = case.n, case.D
    sc = 1.0 if mode == 'int' else 1.0 / np.sqrt(D)
    Uw, Mw = _vals(r, mode, (case.n_user, D)), (_vals(r, mode, (case.n_item, D)) * F32(sc)).astype(F32)
    bu, bi, dy = _vals(r, mode, (case.n_user,)), _vals(r, mode, (case.n_item,)), _vals(r, mode, (n,))
    if mode == 'int':
        z = np.zeros(n, dtype=F32)
    else:
        z = (2.0 * r.randn(n)).astype(F32)
        if case.zmode == 'saturated':
            sat = np.asarray([30.0, -30.0, 100.0, -100.0, 17.0, -17.0, 8.0, -8.0, 20.5, -25.25], dtype=F32)
            z[:min(n, sat.size)] = sat[:n]
    return dict(x=ed_x(case), U=Uw, M=Mw, bu=bu, bi=bi, z=z, dy=dy, mode=mode, case=case, hl=float(F32(ED_HI) - F32(ED_LO)))


def ed_fwd_ref(d):
    "fp64 z, y, their bounds, the flag; a sample with a bad index has z = y = 0"
    case, x = d['case'], d['x']
    ok = (x[:, 0] >= 0) & (x[:, 0] < case.n_user) & (x[:, 1] >= 0) & (x[:, 1] < case.n_item)
    u, it = np.where(ok, x[:, 0], 0), np.where(ok, x[:, 1], 0)
    prod = d['U'].astype(np.float64)[u] * d['M'].astype(np.float64)[it]
    bu, bi = d['bu'].astype(np.float64)[u], d['bi'].astype(np.float64)[it]
    z = np.where(ok, prod.sum(axis=1) + bu + bi, 0.0)
    zb = np.where(ok, U * (cdiv(case.D, 16) + 7) * (np.abs(prod).sum(axis=1) + np.abs(bu) + np.abs(bi)), 0.0)
    if case.has_range:
        with np.errstate(all='ignore'):
            s = 1.0 / (1.0 + np.exp(-z))
        y = np.where(ok, ED_LO + d['hl'] * s, 0.0)
        yb = np.where(ok, d['hl'] * s * (1 - s) * zb + U * (6 * d['hl'] * s + np.abs(y)), 0.0)
    else:
        y, yb = z, zb
    return dict(z=z, zb=zb, y=y, yb=yb, flag=int((~ok).any()))


def check_ed_fwd(d, y, z, flag, ctx=''):
    ref = ed_fwd_ref(d)
    r = collections.OrderedDict()
    if d['mode'] == 'int':
        assert np.abs(d['U']).max(initial=0) * np.abs(d['M']).max(initial=0) * d['case'].D + 8 < 2 ** 24
        if z is not None:
            _same_bits(z, ref['z'].astype(F32), 'z', ctx)
        if not d['case'].has_range:
            _same_bits(y, ref['y'].astype(F32), 'y', ctx)
    if z is not None:
        r['z'] = _ratio(z, ref['z'], ref['zb'], 'z', ctx)
    r['y'] = _ratio(y, ref['y'], ref['yb'], 'y', ctx)
    if flag is not None:
        assert int(flag) == ref['flag'], '%s: err_flag %r' % (ctx, flag)
    return r


ED_MUTANTS = ('drop_sample', 'dU_from_U', 'no_range_factor', 'half_bad_times_zero')


def ed_bwd_ref(d, mutant=None):
    "fp64 dU, dM, dbu, dbi and their bounds (dict name -> (want, bound))"
    case, x = d['case'], d['x']
    ok = (x[:, 0] >= 0) & (x[:, 0] < case.n_user) & (x[:, 1] >= 0) & (x[:, 1] < case.n_item)
    dy, z, hl = d['dy'].astype(np.float64), d['z'].astype(np.float64), d['hl']
    if case.has_range:
        with np.errstate(all='ignore'):
            s = 1.0 / (1.0 + np.exp(-z))
        f = 1.0 if mutant == 'no_range_factor' else hl
        g = dy * f * s * (1 - s)
        gb = U * np.abs(dy) * hl * (9 * s * (1 - s) + 4 * s) + TINY * np.abs(dy) * hl
    else:
        g, gb = dy, np.zeros_like(dy)
    use = ok.copy()
    u, it = x[:, 0], x[:, 1]
    if mutant == 'drop_sample':
        cnt = np.bincount(u[use], minlength=case.n_user)
        b = next(b for b in np.flatnonzero(use)[::-1] if cnt[u[b]] > 1 and g[b] != 0 and d['M'][it[b]].all())
        use[b] = False
    Uw, Mw = d['U'].astype(np.float64), d['M'].astype(np.float64)
    out = {}
    if mutant == 'half_bad_times_zero':                                      # the partner row is read whatever the index says: the arena's NaN
        half = ((u >= 0) & (u < case.n_user)) & ~ok
        nan_rows = np.unique(u[half])
    for name, mine, card, P, partner in (('dU', u, case.n_user, Uw if mutant == 'dU_from_U' else Mw, u if mutant == 'dU_from_U' else it),
                                         ('dM', it, case.n_item, Uw, u)):
        term = g[use, None] * P[partner[use]]
        w, a, e = np.zeros((card, case.D)), np.zeros((card, case.D)), np.zeros((card, case.D))
        np.add.at(w, mine[use], term)
        np.add.at(a, mine[use], np.abs(term))
        np.add.at(e, mine[use], gb[use, None] * np.abs(P[partner[use]]))
        cnt = np.bincount(mine[use], minlength=card).astype(np.float64)
        out[name] = (w, e + U * (cnt[:, None] + 2) * a)
    if mutant == 'half_bad_times_zero' and nan_rows.size:
        out['dU'][0][nan_rows] = np.nan
    for name, mine, card in (('dbu', u, case.n_user), ('dbi', it, case.n_item)):
        w, a, e = np.zeros(card), np.zeros(card), np.zeros(card)
        np.add.at(w, mine[use], g[use])
        np.add.at(a, mine[use], np.abs(g[use]))
        np.add.at(e, mine[use], gb[use])
        cnt = np.bincount(mine[use], minlength=card).astype(np.float64)
        out[name] = (w, e + U * (cnt + 2) * a)
    return out


def ed_int_is_exact(d):
    case = d['case']
    worst = float(np.abs(d['dy']).max(initial=0)) * max(float(np.abs(d['U']).max(initial=0)), float(np.abs(d['M']).max(initial=0)), 1.0) * case.n
    return d['mode'] == 'int' and worst < 2 ** 24 and not d['z'].any() and d['hl'] == 4.0


def check_ed_bwd(d, got, ctx=''):
    "got: dict dU, dM, dbu, dbi.  Returns the ratios (0.0 in int mode: bit for bit)."""
    ref = ed_bwd_ref(d)
    r = collections.OrderedDict()
    for k, (want, bound) in ref.items():
        g = np.asarray(got[k], dtype=F32).reshape(want.shape)
        assert not g[bound == 0].any() and not np.signbit(g[bound == 0]).any(), '%s: %s: an element without a gradient is not +0' % (ctx, k)
        if d['mode'] == 'int':
            assert ed_int_is_exact(d)
            _same_bits(g, want.astype(F32), k, ctx)
            r[k] = 0.0
        else:
            r[k] = _ratio(g.ravel(), want.ravel(), bound.ravel(), k, ctx)
    return r


# ======================================================================================================================================
# nn.Linear with 1 - 4 output features
# ======================================================================================================================================
LIN_SLAB = 64
LIN_DX_GRID = 2048 * 256
LIN_OUTS = ('dx', 'dw', 'db', 'dxdw', 'dxdb', 'dwdb', 'dxdwdb', '')
LinCase = collections.namedtuple('LinCase', 'name M K N ldx_pad bias outs regimes')
LinFacts = collections.namedtuple('LinFacts', 'M K N ldx_pad bias outs nslab lane_steps fwd_passes kblocks bias_alone dx_passes last_slab_rows')


def lin_facts(c):
    return LinFacts(c.M, c.K, c.N, c.ldx_pad, c.bias, c.outs, cdiv(c.M, LIN_SLAB), cdiv(c.K, 64), cdiv(c.K, 512), cdiv(c.K + 1, 64),
                    c.K % 64 == 0, cdiv(c.M * c.K, LIN_DX_GRID), c.M % LIN_SLAB)


LIN_REGIMES = collections.OrderedDict(
    [('N = %d' % n, (lambda n: lambda f: f.N == n)(n)) for n in (1, 2, 3, 4)] +
    [('K = %d' % k, (lambda k: lambda f: f.K == k)(k)) for k in (1, 63, 64, 65, 512, 513)] +
    [('M = %d' % m, (lambda m: lambda f: f.M == m)(m)) for m in (0, 1, 3, 4, 5, 16, 17, 64, 65, 512, 577)] +
    [('outputs: %s' % (o or 'none'), (lambda o: lambda f: f.outs == o)(o)) for o in LIN_OUTS] + [
        ('K < 64: idle lanes', lambda f: f.K < 64),
        ('K = 64 k: the bias column alone in a block of its own', lambda f: f.bias_alone and f.kblocks == f.K // 64 + 1),
        ('K > 512: a second forward pass', lambda f: f.fwd_passes == 2),
        ('nslab = 8: the unrolled final loop alone', lambda f: f.nslab == 8),
        ('nslab = 9: the unrolled final loop and a tail', lambda f: f.nslab == 9),
        ('a partial last slab', lambda f: f.last_slab_rows > 0 and f.nslab > 1),
        ('ldx > K', lambda f: f.ldx_pad > 0),
        ('bias NULL', lambda f: not f.bias),
        ('dx grid-stride: M * K > 2048 * 256', lambda f: f.dx_passes > 1),
    ])
_A = 'outputs: dxdwdb'
LIN_CASES = [
    LinCase('m0', 0, 64, 1, 0, True, 'dxdwdb', ['M = 0', 'K = 64', 'N = 1', _A]),
    LinCase('m1', 1, 1, 1, 0, True, 'dxdwdb', ['M = 1', 'K = 1', 'K < 64: idle lanes']),
    LinCase('m3', 3, 63, 2, 5, True, 'dx', ['M = 3', 'K = 63', 'N = 2', 'ldx > K', 'outputs: dx']),
    LinCase('m4', 4, 64, 3, 0, False, 'dw', ['M = 4', 'N = 3', 'bias NULL', 'outputs: dw', 'K = 64 k: the bias column alone in a block of its own']),
    LinCase('m5', 5, 65, 4, 0, True, 'db', ['M = 5', 'K = 65', 'N = 4', 'outputs: db']),
    LinCase('m16', 16, 512, 1, 0, True, 'dxdw', ['M = 16', 'K = 512', 'outputs: dxdw', 'K = 64 k: the bias column alone in a block of its own']),
    LinCase('m17', 17, 513, 2, 3, True, 'dxdb', ['M = 17', 'K = 513', 'K > 512: a second forward pass', 'outputs: dxdb']),
    LinCase('m64', 64, 63, 3, 0, True, 'dwdb', ['M = 64', 'outputs: dwdb']),
    LinCase('m65', 65, 65, 4, 1, False, '', ['M = 65', 'a partial last slab', 'outputs: none']),
    LinCase('m65-all', 65, 65, 4, 1, False, 'dxdwdb', ['a partial last slab', 'bias NULL', 'ldx > K']),
    LinCase('m512', 512, 64, 1, 0, True, 'dxdwdb', ['M = 512', 'nslab = 8: the unrolled final loop alone']),
    LinCase('m513', 513, 17, 2, 0, True, 'dxdwdb', ['nslab = 9: the unrolled final loop and a tail', 'a partial last slab']),
    LinCase('m577', 577, 65, 3, 2, True, 'dxdwdb', ['M = 577', 'a partial last slab']),
    LinCase('big', 1025, 513, 1, 0, True, 'dxdwdb', ['dx grid-stride: M * K > 2048 * 256']),
]


def lin_data(c, mode):
    r = np.random.RandomState(c.M + c.K + c.N + (0 if mode == 'int' else 1000))
    x = _vals(r, mode, (c.M, c.K + c.ldx_pad))                               # the columns behind K hold values nobody may read
    return dict(x=x, w=_vals(r, mode, (c.N, c.K)), b=_vals(r, mode, (c.N,)) if c.bias else None, dy=_vals(r, mode, (c.M, c.N)), mode=mode, case=c)


LIN_MUTANTS = ('no_bias_column', 'drop_last_slab', 'ldx_as_K')


def lin_ref(d, mutant=None):
    "fp64 y, dx, dw, db with their bounds: dict name -> (want, bound)"
    c = d['case']
    xa = d['x'].astype(np.float64)
    x = xa.ravel()[:c.M * c.K].reshape(c.M, c.K) if mutant == 'ldx_as_K' else xa[:, :c.K]
    w, dy = d['w'].astype(np.float64), d['dy'].astype(np.float64)
    b = np.zeros(c.N) if d['b'] is None else d['b'].astype(np.float64)
    nslab = cdiv(c.M, LIN_SLAB)
    y = x @ w.T + b
    yb = U * (cdiv(c.K, 64) + 8) * (np.abs(x) @ np.abs(w).T + np.abs(b))
    rows = slice(0, LIN_SLAB * (nslab - 1)) if mutant == 'drop_last_slab' else slice(None)
    dw, dwb = dy[rows].T @ x[rows], U * (20 + nslab) * (np.abs(dy).T @ np.abs(x))
    db, dbb = dy[rows].sum(axis=0), U * (20 + nslab) * np.abs(dy).sum(axis=0)
    if mutant == 'no_bias_column':
        db = np.zeros(c.N)
    return dict(y=(y, yb), dx=(dy @ w, U * (c.N + 1) * (np.abs(dy) @ np.abs(w))), dw=(dw, dwb), db=(db, dbb))


def lin_int_is_exact(d):
    c = d['case']
    return d['mode'] == 'int' and 16 * max(c.K, c.M) + 4 < 2 ** 24


def check_lin(d, got, ctx=''):
    "got: dict with any of y, dx, dw, db (None or absent: not produced)"
    ref = lin_ref(d)
    r = collections.OrderedDict()
    for k, (want, bound) in ref.items():
        if got.get(k) is None:
            continue
        g = np.asarray(got[k], dtype=F32).reshape(want.shape)
        if d['mode'] == 'int':
            assert lin_int_is_exact(d)
            _same_bits(g, want.astype(F32), k, ctx)
            r[k] = 0.0
        else:
            r[k] = _ratio(g.ravel(), want.ravel(), bound.ravel(), k, ctx)
    return r


# ======================================================================================================================================
# pad_cols, keep_masks
# ======================================================================================================================================
PadCase = collections.namedtuple('PadCase', 'name rows C Cp regimes')
PAD_REGIMES = collections.OrderedDict([
    ('C = Cp', lambda c: c.C == c.Cp and c.rows > 0),
    ('Cp = C + 3', lambda c: c.Cp == c.C + 3),
    ('rows = 0', lambda c: c.rows == 0),
    ('grid-stride: rows * Cp > 4096 * 256', lambda c: c.rows * c.Cp > TAB_GRID),
])
PAD_CASES = [PadCase('same', 7, 12, 12, ['C = Cp']), PadCase('plus3', 300, 203, 206, ['Cp = C + 3']), PadCase('rows0', 0, 3, 4, ['rows = 0']),
             PadCase('stride', 4100, 254, 257, ['grid-stride: rows * Cp > 4096 * 256', 'Cp = C + 3'])]


def pad_data(c):
    return np.random.RandomState(c.rows + c.C).randn(c.rows, c.C).astype(F32)


def check_pad(c, src, got, ctx=''):
    want = np.zeros((c.rows, c.Cp), dtype=F32)
    want[:, :c.C] = src
    _same_bits(np.asarray(got, dtype=F32).reshape(want.shape), want, 'dst', ctx)


KeepCase = collections.namedtuple('KeepCase', 'name na nb keep_a keep_b regimes')
KEEP_REGIMES = collections.OrderedDict([
    ('u equal to keep gives 0', lambda c: c.na > 2 and c.nb > 2 and c.keep_a < 1 and c.keep_b < 1),
    ('keep = 1', lambda c: c.keep_a == 1.0 or c.keep_b == 1.0),
    ('na = 0', lambda c: c.na == 0 and c.nb > 0),
    ('nb = 0', lambda c: c.nb == 0 and c.na > 0),
    ('grid-stride: na + nb > 4096 * 256', lambda c: c.na + c.nb > TAB_GRID),
])
KEEP_CASES = [KeepCase('both', 300, 77, 0.9, 0.7, ['u equal to keep gives 0']), KeepCase('keep1', 50, 60, 1.0, 0.3, ['keep = 1']),
              KeepCase('na0', 0, 33, 0.9, 0.8, ['na = 0']), KeepCase('nb0', 33, 0, 0.9, 0.8, ['nb = 0']),
              KeepCase('stride', TAB_GRID, 100, 0.99, 0.01, ['grid-stride: na + nb > 4096 * 256', 'u equal to keep gives 0'])]


def keep_data(c):
    "u [na + nb] in [0, 1) with values EQUAL to fl(keep), one ulp below and one above at known places of either part"
    u = np.random.RandomState(c.na + c.nb).rand(c.na + c.nb).astype(F32)
    for off, n, keep in ((0, c.na, c.keep_a), (c.na, c.nb, c.keep_b)):
        if n > 2:
            k = F32(keep)
            u[off], u[off + 1], u[off + 2] = k, np.nextafter(k, F32(0)), min(np.nextafter(k, F32(2)), F32(1.0))
    return u


def keep_ref(c, u, le=False):
    "a, b fp32 (bit for bit); le builds the mutant that keeps u <= keep"
    out = []
    for off, n, keep in ((0, c.na, c.keep_a), (c.na, c.nb, c.keep_b)):
        k = F32(keep)
        part = u[off:off + n]
        out.append(np.where((part <= k) if le else (part < k), F32(1.0) / k, F32(0.0)).astype(F32))
    return out


def check_keep(c, u, a, b, ctx=''):
    wa, wb = keep_ref(c, u)
    if c.na:
        _same_bits(np.asarray(a, dtype=F32), wa, 'a', ctx)
    if c.nb:
        _same_bits(np.asarray(b, dtype=F32), wb, 'b', ctx)


def fmt_ratios(r):
    return '  '.join('%s %.3f' % kv for kv in r.items())
