"""tests/embed_cases.py without a GPU: every case reaches the regime it names and no regime is left without a case; the `int` data are
exact and the renorm inputs keep their margin; the multiply-high division of the scan backward is exact over its whole range; float32
numpy restatements of every kernel's summation order (the sample-order sum of the scans, the SL-slot sum with its xor tree of the sorted
scatter, the lane trees of the forwards, the slab tree of the small linear layer) pass every checker in both modes — the bounds are
reachable by a correct fp32 implementation — and every wrong variant listed in the module is refused."""
import numpy as np
import pytest

import embed_cases as ec

F32 = np.float32
FAMILIES = [(ec.GATHER_CASES, ec.GATHER_REGIMES, ec.tab_facts), (ec.BWD_CASES, ec.BWD_REGIMES, ec.tab_facts),
            (ec.RENORM_CASES, ec.RENORM_REGIMES, ec.renorm_facts), (ec.ED_CASES, ec.ED_REGIMES, ec.ed_facts),
            (ec.LIN_CASES, ec.LIN_REGIMES, ec.lin_facts), (ec.PAD_CASES, ec.PAD_REGIMES, lambda c: c), (ec.KEEP_CASES, ec.KEEP_REGIMES, lambda c: c)]
NAMES = ['gather', 'bwd', 'renorm', 'embdot', 'linear', 'pad', 'keep']
ALL = [(n, c, regimes, facts) for n, (cases, regimes, facts) in zip(NAMES, FAMILIES) for c in cases]


def _case(cases, name):
    return next(c for c in cases if c.name == name)


# ---- the case tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam,case,regimes,facts', ALL, ids=['%s-%s' % (n, c.name) for n, c, _, _ in ALL])
def test_case_reaches_its_regimes(fam, case, regimes, facts):
    f = facts(case)
    assert case.regimes, 'a case names the regime it exists for'
    for name in case.regimes:
        assert regimes[name](f), '%s does not reach "%s": %s' % (case.name, name, f)


@pytest.mark.parametrize('cases,regimes,facts', FAMILIES, ids=NAMES)
def test_census_every_regime_has_a_case(cases, regimes, facts):
    claimed = {name for c in cases for name in c.regimes}
    assert claimed == set(regimes), 'regimes without a case: %s' % sorted(set(regimes) - claimed)
    assert len({c.name for c in cases}) == len(cases)


def test_scan_magic_divides_exactly():
    "e // dj == (e * magic) >> 32 for every dj the scan takes and every staged element e = t + 256 u < 256 * 32"
    e = np.arange(256 * ec.SCAN_MAX_DIM, dtype=np.uint64)
    for dj in range(2, ec.SCAN_MAX_DIM + 1):
        magic = ec.scan_magic(dj)
        assert magic < 2 ** 32 and magic == -(-2 ** 32 // dj)
        assert np.array_equal((e * np.uint64(magic)) >> np.uint64(32), e // np.uint64(dj)), dj
    assert ec.scan_magic(1) == 0                                            # dj = 1 takes e itself


def test_the_plans_hold_what_the_kernels_are_documented_to_skip():
    for c in ec.BWD_CASES + ec.GATHER_CASES:
        if c.invalid:
            x = ec.tab_xcat(c)
            j = 0 if len(c.cards) == 1 else 1
            assert -1 in x[:, j] and c.cards[j] in x[:, j] and ec.TWO32 + min(1, c.cards[j] - 1) in x[:, j]
            assert (x[:, j] == min(1, c.cards[j] - 1)).any(), 'the row that 2^32 + r would alias is in use'
    x = ec.ed_x(_case(ec.ED_CASES, 'd30-600'))
    ok_u, ok_i = (x[:, 0] >= 0) & (x[:, 0] < 300), (x[:, 1] >= 0) & (x[:, 1] < 40)
    assert (ok_u & ~ok_i).sum() == 3 and (~ok_u & ok_i).sum() == 3 and not (~ok_u & ~ok_i).any()


def test_int_data_are_exact_and_renorm_keeps_its_margin():
    for c in ec.BWD_CASES:
        assert ec.tab_int_is_exact(ec.tab_data(c, 'int')), c.name
    for c in ec.ED_CASES:
        assert ec.ed_int_is_exact(ec.ed_data(c, 'int')), c.name
    for c in ec.LIN_CASES:
        assert ec.lin_int_is_exact(ec.lin_data(c, 'int')), c.name
    for c in ec.RENORM_CASES:
        d = ec.renorm_data(c)
        ec.renorm_ref(d)                                                     # asserts the 2^-12 margin
        for w, dj in zip(d['tables'], c.dims):                               # the exact row: 2.25 in fp32 whatever the order
            assert float((w[2].astype(np.float64) ** 2).sum()) == 2.25 and (w[2] * w[2]).sum(dtype=F32) == F32(2.25)


# ---- float32 restatements of the kernels' summation orders ---------------------------------------------------------------------------------
def xor_tree(a, offsets):
    "a[..., lane] += a[..., lane ^ o] for o in offsets, all lanes at once (the __shfl_xor butterflies)"
    lanes = np.arange(a.shape[-1])
    for o in offsets:
        a = (a + a[..., lanes ^ o]).astype(F32)
    return a


def seg_sum_f32(idx, term, card, how):
    """[card, D] fp32: the rows of term [n, D] (fp32, already skipped where idx is -1) added per table row.  how: 'seq' in sample order (the
    scans), 'rev' in reverse order (one arrival order of the atomics), 'slots' the sorted scatter (slot s adds samples s, s + SL, ...,
    then the xor tree over the slots)."""
    n, D = term.shape
    out = np.zeros((card, D), dtype=F32)
    DL, SL = ec.dl_sl(D)
    for row in np.unique(idx[idx >= 0]):
        t = term[idx == row]
        if how == 'rev':
            t = t[::-1]
        if how == 'slots':
            part = np.zeros((SL, D), dtype=F32)
            for q in range(len(t)):
                part[q % SL] = part[q % SL] + t[q]
            # lanes = s * DL + dl: the tree's offsets DL, 2 DL, .. 32 act on the slot number
            out[row] = xor_tree(part.T.copy(), [o // DL for o in (1, 2, 4, 8, 16, 32) if o >= DL and o // DL < SL])[:, 0]
        else:
            acc = np.zeros(D, dtype=F32)
            for v in t:
                acc = acc + v
            out[row] = acc
    return out


def tab_bwd_f32(d, how):
    case, L = d['case'], d['L']
    dtab = np.zeros(L['grad_elems'], dtype=F32)
    for j, (card, dj) in enumerate(zip(case.cards, case.dims)):
        idx = d['x'][:, j]
        idx = np.where((idx >= 0) & (idx < card), idx, -1)
        term = d['dout'][:, L['col_off'][j]:L['col_off'][j] + dj]
        if d['row_mask'] is not None:
            term = (term * d['row_mask'][j][:, None]).astype(F32)
        o = int(L['grad_off'][j])
        dtab[o:o + card * dj] = seg_sum_f32(idx, term, card, how).ravel()
    dcont = None
    if case.n_cont and case.dcont:
        g = d['dout'][:, L['cat_width']:L['cat_width'] + case.n_cont]
        dcont = g if d['cont_mask'] is None else (g * d['cont_mask']).astype(F32)
    return dtab, dcont


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('case', ec.BWD_CASES, ids=ec.case_id)
def test_tab_backward_restated_in_fp32(case, mode):
    d = ec.tab_data(case, mode)
    for how in ('seq', 'slots', 'rev'):
        if case.bs > 4096 and how == 'slots':
            continue
        dtab, dcont = tab_bwd_f32(d, how)
        r = ec.check_tab_bwd(d, dtab, dcont, '%s-%s-%s' % (case.name, mode, how))
        print('RATIO tab_bwd %-8s %-5s %-5s dtab %.3f' % (case.name, mode, how, r))
        assert r <= 1.0


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('mutant', ec.TAB_MUTANTS)
def test_tab_backward_mutants_are_refused(mutant, mode):
    case = _case(ec.BWD_CASES, 'bs513' if mutant in ('drop_last_stage', 'drop_sample') else 'bs257')
    d = ec.tab_data(case, mode)
    want, _, dcont = ec.tab_bwd_ref(d)
    ec.check_tab_bwd(d, want.astype(F32), dcont, 'the reference itself')
    wrong, _, _ = ec.tab_bwd_ref(d, mutant)
    with pytest.raises(AssertionError):
        ec.check_tab_bwd(d, wrong.astype(F32), dcont, mutant)


def test_tab_gather_reference_and_its_mutants():
    for case in ec.GATHER_CASES:
        for mode in ec.MODES:
            d = ec.tab_data(case, mode)
            ec.check_tab_fwd(d, ec.tab_fwd_ref(d))
    d = ec.tab_data(_case(ec.GATHER_CASES, 'mix256'), 'randn')
    with pytest.raises(AssertionError):
        ec.check_tab_fwd(d, ec.tab_fwd_ref(d, pad_nonzero=True), 'pad columns left non-zero')
    alias = dict(d, x=np.where(d['x'] >= ec.TWO32, d['x'] - ec.TWO32, d['x']))
    with pytest.raises(AssertionError):
        ec.check_tab_fwd(d, ec.tab_fwd_ref(alias), 'an index 2^32 + r read as row r')
    other = dict(d, row_mask=np.roll(d['row_mask'], 1, axis=0))
    with pytest.raises(AssertionError):
        ec.check_tab_fwd(d, ec.tab_fwd_ref(other), 'the row mask of another column')


# ---- renorm ---------------------------------------------------------------------------------------------------------------------------------
def renorm_f32(d, ge=False, untouched=False):
    case = d['case']
    out = []
    for j, (card, dj, w) in enumerate(zip(case.cards, case.dims, d['tables'])):
        idx = d['x'][:, j]
        hit = np.bincount(idx[(idx >= 0) & (idx < card)], minlength=card) > 0
        w = w.copy()
        for row in range(card):
            if not (hit[row] or untouched):
                continue
            ss = np.zeros(16, dtype=F32)
            for e in range(dj):
                ss[e % 16] = ss[e % 16] + w[row, e] * w[row, e]
            norm = np.sqrt(xor_tree(ss, (8, 4, 2, 1))[0])
            if (norm >= F32(ec.MAX_NORM)) if ge else (norm > F32(ec.MAX_NORM)):
                w[row] = w[row] * (F32(ec.MAX_NORM) / (norm + F32(1e-7)))
        out.append(w)
    return out


@pytest.mark.parametrize('case', ec.RENORM_CASES, ids=ec.case_id)
def test_renorm_restated_in_fp32_and_its_mutants(case):
    d = ec.renorm_data(case)
    _, flag = ec.renorm_ref(d)
    r = ec.check_renorm(d, renorm_f32(d), flag, np.zeros(4), case.name)
    print('RATIO renorm %-8s %.3f' % (case.name, r))
    assert r <= 1.0
    if case.bs == 0:
        return
    for kw in (dict(ge=True), dict(untouched=True)):
        with pytest.raises(AssertionError):
            ec.check_renorm(d, renorm_f32(d, **kw), flag, np.zeros(4), str(kw))
    with pytest.raises(AssertionError):
        ec.check_renorm(d, renorm_f32(d), 1 - flag, np.zeros(4), 'the flag')
    with pytest.raises(AssertionError):
        ec.check_renorm(d, renorm_f32(d), flag, np.asarray([0, 1]), 'a row flag left set')


# ---- EmbeddingDotBias -----------------------------------------------------------------------------------------------------------------------
def ed_fwd_f32(d):
    case, x = d['case'], d['x']
    n, D = case.n, case.D
    z, y = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    hl = F32(ec.ED_HI) - F32(ec.ED_LO)
    for b in range(n):
        u, it = x[b]
        if not (0 <= u < case.n_user and 0 <= it < case.n_item):
            continue
        acc = np.zeros(16, dtype=F32)
        for e in range(D):
            acc[e % 16] = F32(np.float64(d['U'][u, e]) * np.float64(d['M'][it, e]) + np.float64(acc[e % 16]))       # fmaf
        zz = (xor_tree(acc, (8, 4, 2, 1))[0] + d['bu'][u]) + d['bi'][it]
        z[b] = zz
        with np.errstate(all='ignore'):
            y[b] = F32(ec.ED_LO) + hl * (F32(1) / (F32(1) + np.exp(-zz))) if case.has_range else zz
    return y, z


def ed_g_f32(d):
    case = d['case']
    if not case.has_range:
        return d['dy'].copy()
    hl = F32(ec.ED_HI) - F32(ec.ED_LO)
    with np.errstate(all='ignore'):
        s = (F32(1) / (F32(1) + np.exp(-d['z']).astype(F32))).astype(F32)
    return (d['dy'] * ((hl * s).astype(F32) * (F32(1) - s)).astype(F32)).astype(F32)


def ed_bwd_f32(d, how):
    case, x = d['case'], d['x']
    ok = (x[:, 0] >= 0) & (x[:, 0] < case.n_user) & (x[:, 1] >= 0) & (x[:, 1] < case.n_item)
    g = ed_g_f32(d)
    u, it = np.where(ok, x[:, 0], -1), np.where(ok, x[:, 1], -1)
    tu = (g[:, None] * d['M'][np.maximum(it, 0)]).astype(F32)
    ti = (g[:, None] * d['U'][np.maximum(u, 0)]).astype(F32)
    return dict(dU=seg_sum_f32(u, tu, case.n_user, how), dM=seg_sum_f32(it, ti, case.n_item, how),
                dbu=seg_sum_f32(u, g[:, None], case.n_user, how)[:, 0], dbi=seg_sum_f32(it, g[:, None], case.n_item, how)[:, 0])


ED_CPU_CASES = [c for c in ec.ED_CASES if c.n <= 600]                        # (the large ones differ in the route alone)


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('case', ED_CPU_CASES, ids=ec.case_id)
def test_embdot_restated_in_fp32(case, mode):
    d = ec.ed_data(case, mode)
    y, z = ed_fwd_f32(d)
    r = ec.check_ed_fwd(d, y, z, ec.ed_fwd_ref(d)['flag'], case.name)
    for how in ('seq', 'slots', 'rev'):
        rb = ec.check_ed_bwd(d, ed_bwd_f32(d, how), '%s-%s-%s' % (case.name, mode, how))
        print('RATIO embdot %-12s %-5s %-5s %s  %s' % (case.name, mode, how, ec.fmt_ratios(r), ec.fmt_ratios(rb)))
        assert max(list(r.values()) + list(rb.values())) <= 1.0


def test_saturated_samples_are_asserted_not_excused():
    "at z = 30 the fp32 pass gives g = 0; the reference's g is 9.4e-14 * dy * (hi - lo) and the bound's `4 s` term covers exactly that"
    d = ec.ed_data(_case(ec.ED_CASES, 'n256'), 'randn')
    assert list(d['z'][:4]) == [30.0, -30.0, 100.0, -100.0]
    g = ed_g_f32(d)
    assert g[0] == 0 and g[2] == 0 and g[3] == 0 and g[1] != 0
    d2 = dict(d, z=d['z'].copy())
    d2['z'][4] = F32(2.0)                                                    # a wrong z on one sample (17 -> 2) is far out of bound
    with pytest.raises(AssertionError):
        ec.check_ed_bwd(d, ed_bwd_f32(d2, 'seq'), 'wrong z')


# (int mode with a range has z = 0 and g = dy (hi - lo) / 4: with (hi - lo) missing g is a quarter of an integer, refused as well)
@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('mutant', ec.ED_MUTANTS)
def test_embdot_mutants_are_refused(mutant, mode):
    d = ec.ed_data(_case(ec.ED_CASES, 'd30-600'), mode)
    good = {k: v[0].astype(F32) for k, v in ec.ed_bwd_ref(d).items()}
    ec.check_ed_bwd(d, good, 'the reference itself')
    wrong = {k: v[0].astype(F32) for k, v in ec.ed_bwd_ref(d, mutant).items()}
    with pytest.raises(AssertionError):
        ec.check_ed_bwd(d, wrong, mutant)


# ---- the small linear layer -------------------------------------------------------------------------------------------------------------------
def lin_f32(d, no_bias_column=False, drop_last_slab=False, ldx_as_K=False):
    c = d['case']
    M, K, N = c.M, c.K, c.N
    x = d['x'].ravel()[:M * K].reshape(M, K) if ldx_as_K else d['x'][:, :K]
    w, dy = d['w'], d['dy']
    Kp = ec.cdiv(K, 64) * 64
    y = np.zeros((M, N), dtype=F32)
    for n in range(N):
        prod = np.zeros((M, Kp), dtype=F32)
        prod[:, :K] = x * w[n]
        acc = np.zeros((M, 64), dtype=F32)
        for k0 in range(0, Kp, 64):                                          # lane l adds k = l, l + 64, ... in that order
            acc = acc + prod[:, k0:k0 + 64]
        y[:, n] = xor_tree(acc, (1, 2, 4, 8, 16, 32))[:, 0] + (d['b'][n] if d['b'] is not None else F32(0))
    dx = np.zeros((M, K), dtype=F32)
    for n in range(N):
        dx = dx + dy[:, n:n + 1] * w[n]
    nslab = ec.cdiv(M, ec.LIN_SLAB)
    xb = np.concatenate([x, np.ones((M, 1), dtype=F32)], axis=1)              # the bias column
    dwb = np.zeros((N, K + 1), dtype=F32)
    for s in range(nslab - 1 if drop_last_slab else nslab):
        grp = np.zeros((4, N, K + 1), dtype=F32)
        for g in range(4):
            for m in range(s * 64 + g * 16, min(s * 64 + g * 16 + 16, M)):
                grp[g] = grp[g] + dy[m][:, None] * xb[m][None, :]
        dwb = dwb + (((grp[0] + grp[1]) + grp[2]) + grp[3])
    return dict(y=y, dx=dx, dw=dwb[:, :K].copy(), db=np.zeros(N, dtype=F32) if no_bias_column else dwb[:, K].copy())


LIN_CPU_CASES = [c for c in ec.LIN_CASES if c.M <= 600]


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('case', LIN_CPU_CASES, ids=ec.case_id)
def test_linear_small_restated_in_fp32(case, mode):
    d = ec.lin_data(case, mode)
    r = ec.check_lin(d, lin_f32(d), case.name)
    print('RATIO linear %-8s %-5s %s' % (case.name, mode, ec.fmt_ratios(r)))
    assert max(r.values()) <= 1.0


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('mutant', ec.LIN_MUTANTS)
def test_linear_small_mutants_are_refused(mutant, mode):
    d = ec.lin_data(_case(ec.LIN_CASES, 'm577'), mode)
    with pytest.raises(AssertionError):
        ec.check_lin(d, lin_f32(d, **{mutant: True}), mutant)
    with pytest.raises(AssertionError):
        ec.check_lin(d, {k: v[0].astype(F32) for k, v in ec.lin_ref(d, mutant).items()}, mutant)


# ---- pad_cols, keep_masks ---------------------------------------------------------------------------------------------------------------------
def test_keep_masks_reference_and_its_mutant():
    for c in ec.KEEP_CASES:
        u = ec.keep_data(c)
        a, b = ec.keep_ref(c, u)
        ec.check_keep(c, u, a, b, c.name)
        for part, n, keep in ((a, c.na, c.keep_a), (b, c.nb, c.keep_b)):
            if n > 2:
                assert part[0] == 0 and (part[1] == F32(1) / F32(keep)) == (keep > 0) and part[2] == 0       # u == keep, one ulp below, above
                assert set(np.unique(part)) <= {F32(0), F32(1) / F32(keep)}
    c = _case(ec.KEEP_CASES, 'both')
    u = ec.keep_data(c)
    with pytest.raises(AssertionError):
        ec.check_keep(c, u, *ec.keep_ref(c, u, le=True), ctx='<=')


def test_pad_cols_reference():
    for c in ec.PAD_CASES:
        src = ec.pad_data(c)
        want = np.concatenate([src, np.zeros((c.rows, c.Cp - c.C), dtype=F32)], axis=1)
        ec.check_pad(c, src, want, c.name)
        if c.Cp > c.C and c.rows:
            want[-1, -1] = 1
            with pytest.raises(AssertionError):
                ec.check_pad(c, src, want, c.name)
