"""tests/lstm_cases.py without a GPU: every case takes the route and reaches the regimes it names (through nnl_debug_lstm_plan, which
calls the planner functions of csrc/lstm.hip, lstm_persist.hip and lstm_bptt2.hip themselves), no regime is left without a case, every
template instantiation the planners can reach is named by a case and the rest is unreachable, the fp64 reference agrees with
torch.nn.LSTM under autograd, and the checker of tests/test_lstm_abi_gpu.py rejects five kinds of damaged results."""
import ctypes

import pytest
import torch

import lstm_cases as lc

IDX = list(range(len(lc.CASES)))
ids = lambda i: lc.case_id(lc.CASES[i])


def plan(B, H):
    from neuralnetworklibrary_amd._lib import lib
    out = (ctypes.c_int32 * 14)(*([-7] * 14))
    assert lib.nnl_debug_lstm_plan(B, H, out) == 1
    return lc.Plan(*out)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', IDX, ids=ids)
def test_case_takes_its_route_and_reaches_its_regimes(i):
    c = lc.CASES[i]
    p = plan(c.B, c.H)
    assert lc.routes(c, p) == (c.fwd, c.bwd), '%s: the plan %s sends it to %s' % (lc.case_id(c), p, lc.routes(c, p))
    assert c.regimes, 'a case names the regime it exists for'
    for name in c.regimes:
        assert lc.REGIMES[name](c, p), '%s does not reach "%s": plan %s' % (lc.case_id(c), name, p)


def test_census_every_regime_has_a_case():
    claimed = {name for c in lc.CASES for name in c.regimes}
    assert claimed == set(lc.REGIMES), 'regimes without a case: %s' % sorted(set(lc.REGIMES) - claimed)
    assert len(lc.CASES) <= 45 and len({lc.case_id(c) for c in lc.CASES}) == len(lc.CASES)
    assert {c.T for c in lc.CASES} <= {1, 2, 5, 9} and {c.bwd for c in lc.CHAINED} == {'persist', 'bptt2', 'step'}
    assert all(not c.nulls for c in lc.CHAINED)


def test_every_reachable_instantiation_has_a_case_and_the_rest_is_unreachable():
    """reachable: enumerated from the plan query over 1 <= B <= 128, 1 <= H <= 4096"""
    from neuralnetworklibrary_amd._lib import lib
    out = (ctypes.c_int32 * 14)()
    reach, seen = set(), set()
    for B in range(1, 129):
        for H in range(1, 4097):
            assert lib.nnl_debug_lstm_plan(B, H, out) == 1
            key = tuple(out[6:12])
            if key not in seen:                                              # (ok, U, NWG, ok2, NT, PB): what an instantiation depends on
                seen.add(key)
                reach |= lc.reachable_instantiations(lc.Plan(*out))
            assert out[6] == 0 or out[7] <= 5, 'shape_of accepts U = %d at B = %d, H = %d' % (out[7], B, H)
            assert (B <= 64) or (out[6] == 0 and out[9] == 0)
    assert reach == lc.INSTANTIATED, 'reachable but not instantiated: %s; instantiated but unreachable: %s' % (
        sorted(reach - lc.INSTANTIATED), sorted(lc.INSTANTIATED - reach))
    assert not (reach & lc.UNREACHABLE)
    named = set()
    for c in lc.CASES:
        named |= lc.instantiations(c, plan(c.B, c.H))
    assert named == reach, 'instantiations no case runs: %s' % sorted(reach - named)


def test_plan_query_edges_and_agreement_with_the_older_queries():
    from neuralnetworklibrary_amd._lib import lib
    out = (ctypes.c_int32 * 14)(*([-7] * 14))
    for B, H in ((0, 4), (4, 0), (-1, 4), (4, 1 << 22), (1 << 24, 4)):
        assert lib.nnl_debug_lstm_plan(B, H, out) == 0 and list(out) == [-7] * 14
    assert lib.nnl_debug_lstm_plan(4, 4, None) == 0
    out5 = (ctypes.c_int32 * 5)()
    for B, H in ((64, 1150), (64, 400), (20, 100), (65, 1150), (7, 37), (64, 2048), (64, 1500)):
        p = plan(B, H)
        assert (p.Hp, p.Gp) == (lib.nnl_lstm_padded_hidden(H), lib.nnl_lstm_padded_gates(H))
        assert p.tf == lc.cdiv(B, 64) * lc.cdiv(H, 16) and p.tb == lc.cdiv(B, 64) * lc.cdiv(H, 64)
        assert 1 <= p.sf <= min(32, p.Hp // 32) and 1 <= p.sb <= min(32, p.Gp // 32)
        assert (p.U, p.NWG) == (max(1, lc.cdiv(H, 256)), lc.cdiv(H, max(1, lc.cdiv(H, 256))))
        ok = lib.nnl_debug_lstm_bptt2_plan(B, H, out5)
        assert ok == p.bptt2_ok and (not ok or (out5[0], out5[1], out5[4]) == (p.KG, p.NG, p.NT))
        assert p.PB == (0 if not ok else 8 if p.KG % 8 == 0 else 16)
    # the production shape: 64 x 1150 -> persistent forward <5> on 230 workgroups, lstm_bptt2<5,8> on 16 x 15; per-timestep sf 3, sb 14
    p = plan(64, 1150)
    assert (p.persist_ok, p.U, p.NWG, p.bptt2_ok, p.NT, p.PB, p.KG, p.NG, p.sf, p.sb) == (1, 5, 230, 1, 5, 8, 16, 15, 3, 14)


@pytest.mark.skipif(torch.cuda.is_available(), reason='fake pointers: only where no launch can happen')
def test_a_call_whose_launches_fail_leaves_no_lstm_route_note():
    """the note is written after the launches were issued: where nothing can launch, nothing is noted"""
    from neuralnetworklibrary_amd._lib import lib
    fake = ctypes.c_void_p(0x1000)
    buf = ctypes.create_string_buffer(8192)
    wsb = lib.nnl_lstm_workspace_bytes(2, 4, 37)
    lib.nnl_debug_route_record(1)
    try:
        st_f = lib.nnl_lstm_fwd(fake, fake, fake, fake, fake, fake, fake, 2, 4, 37, fake, wsb, fake, None)
        st_b = lib.nnl_lstm_bwd(fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, 2, 4, 37, fake, wsb, fake, None)
        assert lib.nnl_debug_route_collect(buf, len(buf)) >= 0
    finally:
        lib.nnl_debug_route_record(0)
    assert st_f != 0 and st_b != 0 and b'lstm_' not in buf.value


# ---- the reference against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [i for i in IDX if lc.CASES[i].H <= 256], ids=ids)
def test_reference_agrees_with_torch_lstm_autograd(i):
    """nn.LSTM in fp64 with an identity W_ih and zero biases, fed gx, one timestep per call so that every c_t is seen; the gates
    themselves are not exposed by torch: they are tied through c_t = f c_{t-1} + i g, h_t = o tanh(c_t) and through dgates = d gx"""
    c = lc.CASES[i]
    T, B, H = c.T, c.B, c.H
    d = {k: (None if v is None else v.double()) for k, v in lc.make_inputs(c).items()}
    ref = lc.reference(i)
    m = torch.nn.LSTM(4 * H, H).double()
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(4 * H, dtype=torch.float64)); m.weight_hh_l0.copy_(d['w_hh'])
        m.bias_ih_l0.zero_(); m.bias_hh_l0.zero_()
    gx, h0, c0 = (d[k].clone().requires_grad_(True) for k in ('gx', 'h0', 'c0'))
    h, cc = h0.unsqueeze(0), c0.unsqueeze(0)
    ys, cs = [], []
    for t in range(T):
        y, (h, cc) = m(gx[t:t + 1], (h, cc))
        ys.append(y[0]); cs.append(cc[0])
    y, cy = torch.stack(ys), torch.stack(cs)
    loss = (y * 0).sum()
    if d['dy'] is not None:
        loss = loss + (y * d['dy']).sum()
    if d['dhT'] is not None:
        loss = loss + (h[0] * d['dhT']).sum()
    if d['dcT'] is not None:
        loss = loss + (cc[0] * d['dcT']).sum()
    loss.backward()
    tol = dict(rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref['y'], y.detach(), **tol)
    torch.testing.assert_close(ref['cy'], cy.detach(), **tol)
    torch.testing.assert_close(ref['dgates'], gx.grad, **tol)
    torch.testing.assert_close(ref['dh0'], h0.grad, **tol)
    torch.testing.assert_close(ref['dc0'], c0.grad, **tol)
    g = ref['gates']
    cprev = torch.cat([d['c0'].unsqueeze(0), ref['cy'][:-1]])
    torch.testing.assert_close(g[..., H:2 * H] * cprev + g[..., :H] * g[..., 2 * H:3 * H], ref['cy'], **tol)
    torch.testing.assert_close(g[..., 3 * H:] * torch.tanh(ref['cy']), ref['y'], **tol)
    assert bool(((g[..., :2 * H] > 0) & (g[..., :2 * H] < 1)).all()) and bool((g[..., 2 * H:3 * H].abs() < 1).all())


def test_inputs_keep_the_gates_out_of_saturation():
    """a wrong unit must show: the activations' derivatives are not all ~0"""
    for i in (3, 13, 24):
        g = lc.reference(i)['gates']
        H = lc.CASES[i].H
        assert float((g[..., :H] * (1 - g[..., :H])).median()) > 0.15 and float((1 - g[..., 2 * H:3 * H] ** 2).median()) > 0.3


# ---- the checker can fail ------------------------------------------------------------------------------------------------------------
def as_returned(i):
    """the reference as a perfect kernel would leave it: fp32 numpy arrays, dgates inside the zero-padded [T,B,Gp] tape"""
    c, ref = lc.CASES[i], lc.reference(i)
    p = plan(c.B, c.H)
    out = {k: ref[k].float().numpy().copy() for k in ('y', 'cy', 'gates', 'dh0', 'dc0')}
    tape = torch.zeros(c.T, c.B, p.Gp)
    tape[..., :4 * c.H] = ref['dgates'].float()
    out['dgates_pad'] = tape.numpy().copy()
    return c, ref, p, out


def find(**kw):
    return next(i for i in IDX if all(getattr(lc.CASES[i], k) == v for k, v in kw.items()))


def rejected(out, ref, case, match):
    with pytest.raises(AssertionError, match=match):
        lc.check(out, ref, case)


def test_checker_accepts_the_reference_and_counts_errors_in_tolerances():
    for i in (find(H=515), find(B=65, H=1027), find(H=250)):
        c, ref, p, out = as_returned(i)
        rep = lc.check(out, ref, c)
        assert set(rep) == {'y', 'cy', 'gates', 'dgates', 'dh0', 'dc0'} and all(r[0] < 0.01 for r in rep.values())


def test_checker_rejects_the_last_unit_of_the_last_workgroup_zeroed_at_one_timestep():
    c, ref, p, out = as_returned(find(H=515, bwd='persist'))
    assert c.H - 1 == (p.NWG - 1) * p.U + 1                                 # the second, last live unit of the ragged workgroup
    for name in ('y', 'cy'):
        bad = dict(out)
        bad[name] = out[name].copy()
        bad[name][2, :, c.H - 1] = 0.0
        rejected(bad, ref, c, name + ': max abs err')
    bad = dict(out)
    bad['dgates_pad'] = out['dgates_pad'].copy()
    bad['dgates_pad'][2, :, 3 * c.H + c.H - 1] = 0.0                         # its o gate only
    rejected(bad, ref, c, 'dgates_pad: max abs err')


def test_checker_rejects_a_batch_row_past_64_left_at_the_sentinel():
    c, ref, p, out = as_returned(find(B=65, H=1027))
    for name in ('y', 'gates', 'dgates_pad', 'dh0'):
        bad = dict(out)
        bad[name] = out[name].copy()
        if name == 'dgates_pad':
            bad[name][0, 64, :4 * c.H] = lc.SENTINEL
        else:
            bad[name][..., 64, :] = lc.SENTINEL
        rejected(bad, ref, c, 'never written')


def test_checker_rejects_one_k_slab_dropped_from_dh():
    i = find(H=250, bwd='step')
    c, ref, p, out = as_returned(i)
    assert p.sb == 32
    w = lc.make_inputs(c)['w_hh'].double()
    k = p.Gp // p.sb                                                          # the k range of one slab: 1/sb of dh0 = dgates_0 W_hh
    for s in (0, p.sb // 2):
        bad = dict(out)
        bad['dh0'] = (ref['dh0'] - ref['dgates'][0][:, s * k:(s + 1) * k] @ w[s * k:(s + 1) * k]).float().numpy()
        rejected(bad, ref, c, 'dh0: max abs err')


def test_checker_rejects_dc0_computed_without_dcT():
    for i in (find(T=2, H=257), find(T=9, H=233)):
        c, ref, p, out = as_returned(i)
        d = {k: (None if v is None else v.double()) for k, v in lc.make_inputs(c).items()}
        _, _, dc0 = lc.lstm_backward(d['dy'], d['dhT'], None, ref['gates'], ref['cy'], d['c0'], d['w_hh'])
        bad = dict(out)
        bad['dc0'] = dc0.float().numpy()
        rejected(bad, ref, c, 'dc0: max abs err')


def test_checker_rejects_a_pad_column_that_is_not_exactly_zero():
    c, ref, p, out = as_returned(find(H=250, bwd='step'))
    assert p.Gp > 4 * c.H
    bad = dict(out)
    bad['dgates_pad'] = out['dgates_pad'].copy()
    bad['dgates_pad'][1, 3, p.Gp - 1] = 1e-30
    rejected(bad, ref, c, 'not exactly zero')


def test_fp32_rule_accepts_only_what_fp32_itself_misses_by():
    """beyond the tolerance an output passes only within FP32_FACTOR x the error of the fp32 recurrence on the CPU (+ atol)"""
    i = find(H=250, bwd='step')
    c, ref, p, out = as_returned(i)
    cpu32 = lc.recurrence(c, torch.float32)
    e32 = float((cpu32['dh0'].double() - ref['dh0']).abs().max())
    atol = lc.tolerance('dh0', ref['dh0'])[1]
    bad = dict(out)
    bad['dh0'] = (ref['dh0'] + 50 * (lc.FP32_FACTOR * e32 + atol)).float().numpy()
    with pytest.raises(AssertionError, match='fp32 on the CPU errs by'):
        lc.check(bad, ref, c, cpu32=lambda: cpu32)
    assert e32 < atol, 'at these sizes fp32 itself is far inside the tolerance: the rule has nothing to forgive'
