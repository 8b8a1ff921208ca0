"""tests/text_cases.py without a GPU: every case reaches the launch regime it names and no regime is left without a case; the fp64
references agree with torch in fp64 (F.cross_entropy, F.embedding of W * mask with padding_idx, the AR / TAR expression of the reference's
RegSeqCrossEntropyLoss); fp32 torch on the CPU stays within every softmax-CE bound (the bounds are attainable); the reference rounded to
fp32 passes every comparison of tests/test_text_abi_gpu.py and nine wrong variants of it are refused; and the numpy restatement of the
weight-drop hash keeps the share it should."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import text_cases as tc

F32 = np.float32
FAMILIES = [(tc.CE_CASES, tc.CE_REGIMES, tc.ce_facts), (tc.EMB_CASES, tc.EMB_REGIMES, tc.emb_facts),
            (tc.REG_CASES, tc.REG_REGIMES, tc.reg_facts), (tc.WD_CASES, tc.WD_REGIMES, tc.wd_facts)]
ALL = [(c, regimes, facts) for cases, regimes, facts in FAMILIES for c in cases]


def _case(cases, name):
    return next(c for c in cases if c.name == name)


# ---- the case tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,regimes,facts', ALL, ids=[type(c).__name__ + '-' + c.name for c, _, _ in ALL])
def test_case_reaches_its_regimes(case, regimes, facts):
    f = facts(case)
    assert case.regimes, 'a case names the regime it exists for'
    for name in case.regimes:
        assert regimes[name](f), '%s does not reach "%s": %s' % (case.name, name, f)


@pytest.mark.parametrize('cases,regimes,facts', FAMILIES, ids=['ce', 'emb', 'reg', 'wd'])
def test_census_every_regime_has_a_case(cases, regimes, facts):
    claimed = {name for c in cases for name in c.regimes}
    assert claimed == set(regimes), 'regimes without a case: %s' % sorted(set(regimes) - claimed)
    assert len({c.name for c in cases}) == len(cases)


def test_ce_lane_steps():
    assert tc.ce_lane_steps(768, 0) == (0, 3) and tc.ce_lane_steps(769, 0) == (1, 0) and tc.ce_lane_steps(769, 1) == (0, 3)
    assert tc.ce_lane_steps(1025, 0) == (1, 1) and tc.ce_lane_steps(1025, 1) == (1, 0)
    assert tc.ce_lane_steps(2815, 0) == (2, 3) and tc.ce_lane_steps(2815, 255) == (2, 2) and tc.ce_lane_steps(10, 10) == (0, 0)
    for V in (1, 255, 257, 769, 1500, 47343):                              # every column is read exactly once
        assert sum(4 * u + t for u, t in (tc.ce_lane_steps(V, l) for l in range(256))) == V


def test_ce_targets_cover_the_edges():
    for c in tc.CE_CASES:
        x, t, masked = tc.ce_data(c)
        ok = (t >= 0) & (t < c.V)
        assert np.isfinite(x[np.arange(c.rows)[ok], t[ok]]).all() or c.mode == 'nonfinite'
        if c.rows >= 4 and c.mode in ('randn', 'peaked') and c.V > 2:
            assert 0 in t and c.V - 1 in t and any(t[i] == np.argmax(x[i]) for i in range(c.rows))
        if c.mode == 'masked':
            assert masked.any() and (~masked).any(axis=1).all()
    x, t, masked = tc.ce_data(_case(tc.CE_CASES, 'v700-masked'))
    assert masked[0, [0, 1, 63, 64, 255]].all() and masked[1, :256].all() and masked[2].sum() == 699 and masked[3, 256:512].all()


# ---- the references against torch in fp64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', tc.CE_CASES, ids=tc.case_id)
def test_ce_reference_is_f_cross_entropy(case):
    x, t, _ = tc.ce_data(case)
    ref = tc.ce_reference(x, t, case.gout)
    ok = ref['ok']
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    rows_ok = torch.from_numpy(np.flatnonzero(ok))
    loss = F.cross_entropy(xt[rows_ok], torch.from_numpy(t[ok]), reduction='none')
    (loss.sum() / case.rows).backward(torch.tensor(case.gout, dtype=torch.float64))
    np.testing.assert_allclose(ref['loss'][ok], loss.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref['d'][ok], xt.grad.numpy()[ok], rtol=1e-11, atol=1e-15)
    assert not ref['loss'][~ok].any()
    if case.mode != 'nonfinite':
        np.testing.assert_allclose(ref['mean'], float(loss.sum()) / case.rows, rtol=1e-13)
        np.testing.assert_allclose(ref['p'].sum(axis=1), 1.0, rtol=1e-12)
    else:
        assert np.isnan(ref['loss'][:3]).all() and np.isfinite(ref['loss'][3:]).all() and np.isnan(ref['d'][:3]).all()


def test_ce_reference_is_shift_invariant_and_so_are_its_bounds():
    """the bounds hold no |m| and no |x|: a row shifted by 2^14 and by 2^15 (exactly representable sums) has the same reference and the
    same bounds, and they are those of the unshifted row less the one rounding of m + log s that the kernel makes for |m| <= 16"""
    r = np.random.RandomState(3)
    x = np.round(3 * r.randn(5, 300) * 256) / 256
    t = np.asarray([0, 299, 5, 17, 100])
    for sh in (16384.0, 32768.0):
        assert np.array_equal((x + sh).astype(F32).astype(np.float64), x + sh)
    o, a, b = (tc.ce_reference((x + sh).astype(F32), t, 2.5) for sh in (0.0, 16384.0, 32768.0))
    for k in ('logs', 'loss', 'd', 'logs_bound', 'loss_bound', 'd_bound'):
        assert np.array_equal(a[k], b[k]), k
    for k in ('logs', 'loss', 'd', 'logs_bound'):
        assert np.array_equal(o[k], a[k]), k
    assert (np.abs(o['m']) <= tc.CE_LSE_JOIN).all()
    np.testing.assert_allclose(o['loss_bound'] - a['loss_bound'], tc.U * (tc.CE_LSE_JOIN + np.abs(o['logs'])), rtol=1e-9)
    assert (o['d_bound'] >= a['d_bound']).all()


def test_ce_cases_take_both_forms_of_lse():
    "rows on either side of |m| = 16, where the kernels join m + log s or keep them apart, at ordinary magnitudes and at the offsets"
    side = {}
    for c in tc.CE_CASES:
        x, t, _ = tc.ce_data(c)
        m = np.fmax.reduce(x.astype(np.float64), axis=1)
        m = m[np.isfinite(m)]
        side.setdefault(c.mode.rstrip('+-0123456789'), []).extend((np.abs(m) <= tc.CE_LSE_JOIN).tolist())
    assert all(side['randn']) and all(side['masked']) and not any(side['peaked']) and not any(side['offset'])


@pytest.mark.parametrize('mode', tc.EMB_MODES)
@pytest.mark.parametrize('case', tc.EMB_CASES, ids=tc.case_id)
def test_embedding_reference_is_f_embedding(case, mode):
    d = tc.emb_data(case, mode)
    x, V = d['x'], case.V
    ok = (x >= 0) & (x < V)
    W = torch.from_numpy(d['W'].astype(np.float64)).requires_grad_()
    rm = torch.ones(V, dtype=torch.float64) if d['rowmask'] is None else torch.from_numpy(d['rowmask'].astype(np.float64))
    out = F.embedding(torch.from_numpy(x[ok]), W * rm[:, None], None if d['pad'] < 0 else d['pad'])
    out.backward(torch.from_numpy(d['dout'].astype(np.float64)[ok]))
    got, flag = tc.emb_fwd_ref(d)
    assert flag == int((~ok).any()) and not got[~ok].any()
    assert np.array_equal(tc.bits(got[ok]), tc.bits(out.detach().numpy().astype(F32)))
    dW, bound = tc.emb_bwd_ref(d)
    np.testing.assert_allclose(dW, W.grad.numpy(), rtol=1e-12, atol=1e-12)
    if d['pad'] >= 0:
        assert not dW[d['pad']].any()
    assert tc.check_emb_bwd(d, dW.astype(F32)) <= 1.0                      # the reference rounded to fp32 passes
    if mode == 'int':
        assert np.array_equal(dW, np.round(dW))


@pytest.mark.parametrize('ab', tc.REG_AB, ids=lambda ab: 'a%g-b%g' % ab)
@pytest.mark.parametrize('mode', tc.REG_MODES)
@pytest.mark.parametrize('case', tc.REG_CASES, ids=tc.case_id)
def test_seq_reg_reference_is_the_ar_tar_expression(case, mode, ab):
    alpha, beta = ab
    h = tc.reg_data(case, mode)
    ht = torch.from_numpy(h.astype(np.float64)).requires_grad_()
    ar = ht.pow(2).mean()
    tar = (ht[1:] - ht[:-1]).pow(2).mean() if case.T > 1 else torch.zeros((), dtype=torch.float64)
    (alpha * ar + beta * tar).backward(torch.tensor(2.5, dtype=torch.float64))
    ref = tc.reg_reference(h, alpha, beta, 2.5)
    np.testing.assert_allclose([ref['ar'], ref['tar']], [float(ar), float(tar)], rtol=1e-12)
    np.testing.assert_allclose(ref['dh'], ht.grad.numpy(), rtol=1e-11, atol=1e-18)
    out3 = np.asarray([alpha * ref['ar'] + beta * ref['tar'], ref['ar'], ref['tar']]).astype(F32)
    r = tc.check_reg(h, alpha, beta, 2.5, mode, out3, ref['dh'].astype(F32))
    assert max(r.values()) <= 1.0
    if mode == 'dyadic':
        assert float((h.astype(np.float64) ** 2).sum()) < 2 ** 24 and 4 * float((h.astype(np.float64) ** 2).sum()) < 2 ** 24


# ---- the bounds are attainable: fp32 torch on the CPU stays within them -------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in tc.CE_CASES if c.mode != 'badtarget'], ids=tc.case_id)
def test_fp32_torch_meets_the_ce_bounds(case):
    """F.cross_entropy and its autograd in fp32 (torch refuses a target outside [0, V), so not the bad-target case).  The NaN rows of the
    non-finite case are NaN in torch too, and the -inf columns of the masked cases get exactly zero gradient."""
    x, t, masked = tc.ce_data(case)
    xt = torch.from_numpy(x).requires_grad_()
    tt = torch.from_numpy(t)
    rows_loss = F.cross_entropy(xt, tt, reduction='none')
    mean = F.cross_entropy(xt, tt)
    mean.backward(torch.tensor(case.gout))
    ld = tc.ce_ld(case.V, case.ld)
    d = np.zeros((case.rows, ld), dtype=F32)
    d[:, :case.V] = xt.grad.numpy()
    stats = None
    if case.mode != 'nonfinite':
        with torch.no_grad():
            m = xt.max(dim=1).values
            stats = torch.stack([m, torch.log(torch.exp(xt - m[:, None]).sum(dim=1))], dim=1).numpy()
    got = dict(stats=stats, loss_rows=rows_loss.detach().numpy(), mean=mean.item(), d=d, err_flag=0)
    r = tc.check_ce(case, x, t, masked, got, case.name)
    print('RATIO fp32 torch %-18s %s' % (case.name, tc.fmt_ratios(r)))
    assert max(r.values()) <= 1.0


# ---- mutants: the reference rounded to fp32 passes, each wrong variant is refused -----------------------------------------------------------
def _ce_pair(name):
    case = _case(tc.CE_CASES, name)
    x, t, masked = tc.ce_data(case)
    ref = tc.ce_reference(x, t, case.gout)
    got = tc.ce_result_from(ref, tc.ce_ld(case.V, case.ld), case.rows)
    assert max(tc.check_ce(case, x, t, masked, got, name).values()) <= 1.0
    return case, x, t, masked, ref, got


@pytest.mark.parametrize('case', tc.CE_CASES, ids=tc.case_id)
def test_ce_reference_rounded_to_fp32_passes(case):
    _ce_pair(case.name)


def _refused(check, *a):
    with pytest.raises(AssertionError):
        check(*a)


def test_mutant_onehot_one_column_early():
    case, x, t, masked, ref, got = _ce_pair('v300')
    d = ref['p'].copy()
    for i in range(case.rows):
        d[i, (t[i] - 1) % case.V] -= 1.0
    got['d'][:, :case.V] = (d * case.gout / case.rows).astype(F32)
    _refused(tc.check_ce, case, x, t, masked, got)


def test_mutant_mean_over_rows_minus_one():
    case, x, t, masked, ref, got = _ce_pair('v300')
    got['mean'] = F32(got['loss_rows'].astype(np.float64).sum() / (case.rows - 1))
    _refused(tc.check_ce, case, x, t, masked, got)


def test_mutant_a_tail_column_dropped_from_the_sum():
    case, x, t, masked, ref, got = _ce_pair('v300')
    assert tc.ce_lane_steps(case.V, case.V - 1 - 256)[1] == 2              # the last column is a second tail step
    x64 = x.astype(np.float64)
    s = np.exp(x64 - ref['m'][:, None])[:, :-1].sum(axis=1)
    got['stats'][:, 1] = np.log(s).astype(F32)
    _refused(tc.check_ce, case, x, t, masked, got)
    got = tc.ce_result_from(ref, tc.ce_ld(case.V, case.ld), case.rows)
    got['loss_rows'] = (ref['loss'] + np.log(s) - ref['logs']).astype(F32)
    _refused(tc.check_ce, case, x, t, masked, got)
    got = tc.ce_result_from(ref, tc.ce_ld(case.V, case.ld), case.rows)
    got['d'][:, :case.V] = ((np.exp(x64 - ref['m'][:, None] - np.log(s)[:, None]) - (ref['p'] - ref['d'] * case.rows / case.gout))
                            * case.gout / case.rows).astype(F32)
    _refused(tc.check_ce, case, x, t, masked, got)


def test_mutant_pad_columns_left_unwritten():
    case, x, t, masked, ref, got = _ce_pair('v300')
    assert tc.ce_ld(case.V, case.ld) > case.V
    got['d'][3, case.V + 1] = 12345.0
    _refused(tc.check_ce, case, x, t, masked, got)
    got['d'][3, case.V + 1] = -0.0
    _refused(tc.check_ce, case, x, t, masked, got)


@pytest.mark.parametrize('name', ['v300-off+20000', 'v300-off+1000', 'v200-off', 'v768', 'v1500-off', 'v2048', 'v47343-off'])
def test_mutant_lse_rounded_as_one_number(name):
    """l = fl(m + log s), loss = fl(l - x_t), p = exp(fl(x - l)): the kernels before row_stats = {m, log s}.  The offset cases refuse
    both the loss and the gradient."""
    case, x, t, masked, ref, got = _ce_pair(name)
    lse = (ref['m'] + ref['logs']).astype(F32)
    x_t = x[np.arange(case.rows), t]
    bad = dict(got, loss_rows=(lse - x_t).astype(F32), d=got['d'].copy())
    _refused(tc.check_ce, case, x, t, masked, bad)
    arg = (x - lse[:, None]).astype(F32).astype(np.float64)
    onehot = ref['p'] - ref['d'] * case.rows / case.gout
    bad = dict(got, d=got['d'].copy())
    bad['d'][:, :case.V] = ((np.exp(arg) - onehot) * case.gout / case.rows).astype(F32)
    _refused(tc.check_ce, case, x, t, masked, bad)


@pytest.mark.parametrize('mode', tc.EMB_MODES)
def test_mutant_padding_row_receives_gradient(mode):
    d = tc.emb_data(_case(tc.EMB_CASES, 'd3'), mode)
    assert d['pad'] >= 0 and (d['x'] == d['pad']).any()
    _refused(tc.check_emb_bwd, d, tc.emb_bwd_ref(d, pad_gets_gradient=True)[0].astype(F32))


@pytest.mark.parametrize('mode', tc.EMB_MODES)
@pytest.mark.parametrize('row', [2, 3, 39])
def test_mutant_one_sample_of_a_segment_missing(mode, row):
    "rows 2, 3 and 39 of case d3 hold SL + 1, 70 and 193 samples"
    d = tc.emb_data(_case(tc.EMB_CASES, 'd3'), mode)
    assert (d['x'] == row).sum() in (17, 70, 193)
    _refused(tc.check_emb_bwd, d, tc.emb_bwd_ref(d, drop_one_of_row=row)[0].astype(F32))


@pytest.mark.parametrize('mode', tc.REG_MODES)
def test_mutant_tar_across_the_unroll_seam(mode):
    "t = 9 is the first step of the second unrolled pass: its difference taken against h[7]"
    case = _case(tc.REG_CASES, 't17')
    h = tc.reg_data(case, mode)
    good, bad = tc.reg_reference(h, 0.0, 1.0), tc.reg_reference(h, 0.0, 1.0, seam_mutant=True)
    out3 = lambda r: np.asarray([r['tar'], r['ar'], r['tar']]).astype(F32)
    assert max(tc.check_reg(h, 0.0, 1.0, 1.0, mode, out3(good), good['dh'].astype(F32)).values()) <= 1.0
    _refused(tc.check_reg, h, 0.0, 1.0, 1.0, mode, out3(bad), good['dh'].astype(F32))
    _refused(tc.check_reg, h, 0.0, 1.0, 1.0, mode, out3(good), bad['dh'].astype(F32))


def test_mutant_out3_components_swapped_or_missing():
    h = tc.reg_data(_case(tc.REG_CASES, 't10'), 'randn')
    ref = tc.reg_reference(h, 2.0, 1.0)
    v = 2.0 * ref['ar'] + ref['tar']
    _refused(tc.check_reg, h, 2.0, 1.0, 1.0, 'randn', np.asarray([v, ref['tar'], ref['ar']]).astype(F32), None)
    _refused(tc.check_reg, h, 2.0, 1.0, 1.0, 'randn', np.asarray([v, ref['ar'], 0.0]).astype(F32), None)


def test_mutant_hash_indexed_by_the_padded_row():
    c = _case(tc.WD_CASES, 'hash-.25')
    assert tc.wd_ld_out(c.H, c.ld_out) != c.H
    src, mask = tc.wd_data(c)
    tc.check_wd(c, src, mask, tc.wd_reference(c, src, mask)[0])
    _refused(tc.check_wd, c, src, mask, tc.wd_reference(c, src, mask, index_by_ld_out=True)[0])


@pytest.mark.parametrize('case', tc.WD_CASES, ids=tc.case_id)
def test_weight_drop_reference_passes_and_a_written_pad_column_is_refused(case):
    src, mask = tc.wd_data(case)
    out, _ = tc.wd_reference(case, src, mask)
    tc.check_wd(case, src, mask, out)
    if out.shape[1] > case.H:
        out[-1, -1] = 1.0
        _refused(tc.check_wd, case, src, mask, out)


# ---- the restated hash ----------------------------------------------------------------------------------------------------------------------
def test_splitmix64_restatement():
    "the first outputs of splitmix64 from state 0 (Vigna's reference values): wd_keep's mixer with seed + idx * golden as the state"
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for i, w in enumerate(want):
        top = w >> 40
        for p, keep in ((0.0, True), (top / 2.0 ** 24, True), ((top + 1) / 2.0 ** 24, False)):
            assert bool(tc.wd_keep(0, [i + 1], p)[0]) == keep


@pytest.mark.parametrize('p', tc.WD_P)
@pytest.mark.parametrize('seed', tc.WD_SEEDS)
def test_hash_keeps_the_share_it_should(seed, p):
    keep = tc.wd_keep(seed, np.arange(4600 * 1150 // 8), p)
    assert tc.wd_share_sigmas(keep, p) < 5.0
    rows = keep[:574 * 1150].reshape(574, 1150)                             # no row or column pattern either
    assert abs(rows.mean(axis=0) - (1 - p)).max() < 6 * np.sqrt(p * (1 - p) / 574)
    assert abs(rows.mean(axis=1) - (1 - p)).max() < 6 * np.sqrt(p * (1 - p) / 1150)
