"""tests/retina_cases.py without a GPU: every regime of the detection-loss sweep has a case, every case's reference state holds what the
case was built for (positives, ignored, the all-padding image, the image without a positive; the IoU-1/2, IoU-2/5, tie, zero-area and
tw-clamp constructions land where intended), a correct fp32 evaluation fits the tolerances the kernel will be judged by, the new
reference reproduces the reference project's own run (golden G8), the float index trick of the class stream is exact, and the C entry
points refuse what the header says they refuse — before any HIP call, so that runs here."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import retina_cases as rc
from conftest import assert_close, load_golden

IDX = list(range(len(rc.CASES)))
ids = lambda i: rc.CASES[i].name
f32 = np.float32


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
def test_census_every_regime_has_a_case():
    cov = rc.coverage()
    for k, names in cov.items():
        _say('RETINA_REGIME %-55s %s' % (k, ' '.join(names)))
    assert not [k for k, names in cov.items() if not names], 'regimes without a case: %s' % [k for k, v in cov.items() if not v]
    assert 25 <= len(rc.CASES) <= 30 and len({c.name for c in rc.CASES}) == len(rc.CASES)
    assert max(c.bs * c.A * c.K for c in rc.CASES) == 16385 * 4, 'the 16385-anchor case holds the largest tensor'
    assert all(0 <= c.M <= rc.KMAXOBJ and 1 <= c.K <= 4096 for c in rc.CASES)
    assert {rc.case(n).K % 4 != 0 for n in rc.CHAINED} == {True, False}
    assert any(rc.case(n).K % 4 == 0 and rc.case(n).K > 32 for n in rc.CHAINED) and any(rc.case(n).K in (4, 20) for n in rc.CHAINED)
    assert rc.case(rc.ALONE).bs == 17 and rc.case(rc.PERMUTED).pad == 'inter'


@pytest.mark.parametrize('i', IDX, ids=ids)
def test_inputs_are_valid_and_exactly_representable(i):
    """what the kernel relies on and no test may violate: cats in [0, K) or -1, positive anchor areas, and the dyadic grid"""
    c = rc.CASES[i]
    d = rc.make_inputs(c)
    a = d['anchors']
    assert a.dtype == f32 and a.shape == (c.A, 4) and ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) > 0).all()
    assert (a * 8 == np.round(a * 8)).all() and (a >= 0).all() and (a < 64).all()
    wh = np.concatenate([a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]])
    assert set(np.unique(wh)) <= set(rc.SIZES) | {5.0} and (wh == 5.0).sum() == 1
    assert d['cats'].dtype == np.int64 and d['cats'].shape == (c.bs, c.M) and ((d['cats'] == -1) | ((d['cats'] >= 0) & (d['cats'] < c.K))).all()
    assert d['boxes'].shape == (c.bs, c.M, 4) and (d['boxes'] * 8 == np.round(d['boxes'] * 8)).all()
    assert (d['boxes'][d['cats'] < 0] == -1).all()
    assert d['clas'].dtype == f32 and ((d['clas'] >= 0) & (d['clas'] <= 1)).all() and np.isfinite(d['reg']).all()


@pytest.mark.parametrize('i', IDX, ids=ids)
def test_reference_state_holds_what_the_case_was_built_for(i):
    c = rc.CASES[i]
    d, r = rc.make_inputs(c), rc.reference(c)
    A = c.A
    iH, iF, iS, iT = 0, 1, A - 2, A - 1
    assert tuple(d['anchors'][iT]) == rc.ANCH_T and tuple(d['anchors'][iS]) == rc.ANCH_S and tuple(d['anchors'][iF]) == rc.ANCH_F
    for img in range(c.bs):
        kind, st = rc.kind_of(c, img), r['state'][img]
        valid = d['cats'][img] >= 0
        objs, cats = d['boxes'][img][valid], d['cats'][img][valid]
        assert r['npos'][img] == (st >= 0).sum()
        if kind in ('null', 'allpad'):
            assert not valid.any() and (st == -1).all() and r['npos'][img] == 0
            continue
        assert valid.any() and (st[st >= 0] < len(objs)).all()
        if kind == 'nopos':
            assert r['npos'][img] == 0 and st[iH] == -2 and st[iF] == -2 and (st == -1).sum() == A - 2
            continue
        assert (st >= 0).any() and (st == -1).any()
        if kind == 'rand':
            last = len(objs) - 1                                      # the last valid row copies an anchor of its own
            assert (st == last).any()
            continue
        assert kind == 'full' and c.M >= 8 and (st == -2).any()
        rows = {name: [j for j, o in enumerate(objs) if tuple(o) == tuple(float(v) for v in box)] for name, box in (
            ('half', rc.OBJ_HALF), ('twofifths', rc.OBJ_TWOFIFTHS), ('T', rc.ANCH_T), ('zero', rc.OBJ_ZERO), ('S', rc.ANCH_S))}
        assert [len(rows[k]) for k in ('half', 'twofifths', 'T', 'zero', 'S')] == [1, 1, 2, 1, 1]
        assert st[iH] == -2 and st[iF] == -2, 'IoU exactly 1/2 and exactly fp32(2/5) are both ignored'
        t1, t2 = rows['T']
        assert st[iT] == t1 < t2, 'two identical objects: the lower row wins'
        if c.K > 1:
            assert cats[t1] != cats[t2] and r['tcls'][img, iT] == cats[t1]
        assert not (st == rows['zero'][0]).any(), 'a zero-area object matches nothing'
        assert st[iS] == rows['S'][0]
        tw = r['target'][img, iS]
        want = np.log(1 / 0.75) / float(f32(0.2))                     # tw = th = 0.75 clamped to 1 over a 0.75 anchor
        assert tw[0] == 0 and tw[1] == 0 and abs(tw[2] - want) < 1e-12 and abs(tw[3] - want) < 1e-12
    if c.M == 128:
        assert rc.REGIMES['objects M=128 both halves, positive from the second'](c, d, r)


def test_threshold_constructions_sit_exactly_on_the_thresholds():
    half, two5 = rc.iou32(rc.ANCH_H, rc.OBJ_HALF), rc.iou32(rc.ANCH_F, rc.OBJ_TWOFIFTHS)
    assert half == f32(0.5) and not half > f32(0.5)
    assert two5 == f32(0.4) and not two5 < f32(0.4) and float(two5) > 0.4      # fp32(2/5) lies above 2/5: a double comparison would differ
    assert rc.iou32(rc.ANCH_H, rc.OBJ_ZERO) == 0 and rc.iou32(rc.ANCH_T, rc.ANCH_T) == 1
    st = rc.match32(np.array([rc.ANCH_H, rc.ANCH_F, rc.ANCH_T], f32), np.array([rc.OBJ_ZERO, rc.OBJ_HALF, rc.OBJ_TWOFIFTHS, rc.ANCH_T, rc.ANCH_T], f32))
    assert list(st) == [-2, -2, 3]
    assert list(rc.match32(np.array([rc.ANCH_H], f32), np.zeros((0, 4), f32))) == [-1]


def test_inputs_reach_the_edges_over_the_table():
    """over all cases: every exact clas value on a target class, on another class and on an ignored anchor; both ends of the clamp range
    on live elements; both Huber branches with both signs, the knee from either side and a zero difference"""
    seen = {(float(v), w): 0 for v in rc.EXACT_CLAS for w in ('target', 'other', 'ignored')}
    huber = dict(quad_pos=0, quad_neg=0, lin_pos=0, lin_neg=0, knee_below=0, knee_above=0, zero=0)
    for c in rc.CASES:
        d, r = rc.make_inputs(c), rc.reference(c)
        ign = np.broadcast_to((r['state'] == -2)[:, :, None], d['clas'].shape)
        for v in rc.EXACT_CLAS:
            hit = d['clas'] == v
            seen[(float(v), 'target')] += int((hit & r['is_target'] & ~ign).sum())
            seen[(float(v), 'other')] += int((hit & ~r['is_target'] & ~ign).sum())
            seen[(float(v), 'ignored')] += int((hit & ign).sum())
        pos = r['state'] >= 0
        diff = (r['target'] - d['reg'].astype(np.float64))[pos]
        ad = np.abs(diff)
        huber['quad_pos'] += int(((ad < 0.1) & (diff > 1e-3)).sum()); huber['quad_neg'] += int(((ad < 0.1) & (diff < -1e-3)).sum())
        huber['lin_pos'] += int((diff > 0.5).sum()); huber['lin_neg'] += int((diff < -0.5).sum())
        huber['knee_below'] += int(((ad > 1 / 9 - 2e-3) & (ad < 1 / 9)).sum()); huber['knee_above'] += int(((ad >= 1 / 9) & (ad < 1 / 9 + 2e-3)).sum())
        huber['zero'] += int((ad < 1e-6).sum())
    _say('RETINA_EDGES clas', {k: v for k, v in seen.items()})
    _say('RETINA_EDGES huber', huber)
    assert all(v > 0 for v in seen.values()), [k for k, v in seen.items() if v == 0]
    assert all(v > 0 for v in huber.values()), huber


# ---- the tolerances hold for a correct fp32 evaluation ------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize('i', IDX, ids=ids)
def test_fp32_restatement_sits_inside_the_tolerances(i):
    c = rc.CASES[i]
    d, r = rc.make_inputs(c), rc.reference(c)
    s = rc.restate32(c, d, r)
    q_out = rc.check_forward(c, r, r['state'], r['npos'], s['out'], ' (numpy fp32)')
    q_reg, q_clas = rc.check_backward(c, r, s['dreg'], s['dclas'], ' (numpy fp32)')
    pos = r['state'] >= 0
    q_enc = 0.0
    if pos.any():                                                      # the encoding alone: |t32 - t64| against dt
        t32 = np.zeros_like(r['target'])
        for img in range(c.bs):
            p = np.nonzero(pos[img])[0]
            if len(p):
                valid = d['cats'][img] >= 0
                t32[img, p] = rc.encode32(d['anchors'][p], d['boxes'][img][valid][r['state'][img][p]])
        q_enc = float((np.abs(t32 - r['target']) / r['dt'])[pos].max())
    WORST[c.name] = (q_out, q_reg, q_clas, q_enc)
    _say('RETINA_FP32 %-22s err / tolerance: out %.3f dreg %.3f dclas %.3f, encoding error / dt %.3f' % (c.name, q_out, q_reg, q_clas, q_enc))
    assert q_enc <= 1.0
    if len(WORST) == len(rc.CASES):
        _say('RETINA_FP32 worst over the table: out %.3f dreg %.3f dclas %.3f encoding %.3f' % tuple(max(w[k] for w in WORST.values()) for k in range(4)))


def as_returned(name):
    c = rc.case(name)
    r = rc.reference(c)
    return c, r, r['dreg'].astype(f32), r['dclas'].astype(f32)


def test_checker_rejects_damaged_results():
    c, r, dreg, dclas = as_returned('k3-a257-m8')
    assert max(rc.check_backward(c, r, dreg, dclas)) < 0.1
    live_other = np.argwhere(r['live'] & ~r['is_target'] & (r['clas'] < 1e-2) & (r['clas'] > rc.LO))
    assert len(live_other)
    bad = dclas.copy(); bad[tuple(live_other[0])] *= f32(1.002)        # a small-probability negative class 2e-3 off: an atol sized to the tensor hides it
    with pytest.raises(AssertionError, match='dclas'):
        rc.check_backward(c, r, dreg, bad)
    bad = dclas.copy(); bad[1, 256, 2] = 0.0                            # the last element of the one-anchor tail chunk left unwritten (zero)
    assert r['live'][1, 256, 2]
    with pytest.raises(AssertionError, match='dclas'):
        rc.check_backward(c, r, dreg, bad)
    outside = np.argwhere(~r['inside'] & (r['state'] != -2)[:, :, None])
    bad = dclas.copy(); bad[tuple(outside[0])] = f32(1e-30)
    with pytest.raises(AssertionError, match='not exactly 0'):
        rc.check_backward(c, r, dreg, bad)
    bad = dreg.copy(); bad[0, 5, 1] = f32(1e-30)
    assert r['state'][0, 5] < 0
    with pytest.raises(AssertionError, match='dreg is not exactly 0'):
        rc.check_backward(c, r, bad, dclas)
    p = tuple(np.argwhere(np.abs(r['dreg']) > 0)[0])
    bad = dreg.copy(); bad[p] *= f32(1.001)
    with pytest.raises(AssertionError, match='dreg'):
        rc.check_backward(c, r, bad, dclas)
    st = r['state'].copy(); st[0, 0] = -1                               # IoU exactly 1/2 filed as negative
    with pytest.raises(AssertionError, match='state differs'):
        rc.check_forward(c, r, st, r['npos'], r['out'].astype(f32))
    out = r['out'].astype(f32); out[2] *= f32(1.0001)
    with pytest.raises(AssertionError, match='out'):
        rc.check_forward(c, r, r['state'], r['npos'], out)


# ---- the reference against the reference project's own run -----------------------------------------------------------------------------------
def test_reference_reproduces_golden_g8():
    """golden G8 (the reference project's fp32 run on anchors_for(64, 64), three images, one without objects): the states exactly, the
    losses and gradients at the tolerances of test_detection.py::test_g8_loss_oracle"""
    from oracle import reference_math as RM
    g = load_golden('g8_detection')
    anchors = RM.anchors_for(64, 64).numpy()
    r = rc.reference_of(anchors, g['reg'], g['clas'], g['boxes'], g['cats'], 0.5, 0.25, 2.0, 1.0)
    for i in range(len(g['boxes'])):
        st = np.full(len(anchors), -2, dtype=np.int64)
        st[g['img%d.neg' % i]] = -1
        pos = g['img%d.pos' % i]
        st[pos] = g['img%d.matches' % i][pos]
        np.testing.assert_array_equal(r['state'][i], st)
        assert_close(r['img_reg'][i], g['img%d.reg_loss' % i], 1e-6, 1e-7, 'img reg')
        assert_close(r['img_clas'][i], g['img%d.clas_loss' % i], 1e-6, 1e-7, 'img clas')
    assert_close(r['out'][0], g['loss'], 1e-6, 1e-7, 'loss')
    assert_close(r['out'][1], g['reg_loss'], 1e-6, 1e-7, 'reg')
    assert_close(r['out'][2], g['clas_loss'], 1e-6, 1e-7, 'clas')
    assert_close(r['dreg'], g['dreg'], 1e-5, 1e-9, 'dreg')
    assert_close(r['dclas'], g['dclas'], 1e-5, 1e-9, 'dclas')


# ---- the float index trick of the class stream ------------------------------------------------------------------------------------------------
def _anchor_of(e, K):
    "int((float(e) + 0.5f) * (1.f / float(K))) as retina_loss.hip computes it"
    inv_k = f32(1) / f32(K)
    return ((e.astype(f32) + f32(0.5)) * inv_k).astype(np.int32)


def test_float_index_of_an_element_is_its_anchor_for_every_k():
    """for K in 1 .. 4096 and every element e < 256 K of a chunk, int((e + .5f) * (1f / K)) == e // K.  The expression is non-decreasing
    in e (an exact conversion, a rounded addition, a rounded multiplication by a positive constant, a truncation), so it equals e // K on
    all of [nK, (n+1)K) as soon as it does on both ends: those are checked for every K and n; for K <= 128 and the largest K every
    element is checked as well."""
    n = np.arange(256, dtype=np.int64)
    for K in range(1, 4097):
        first, last = n * K, n * K + (K - 1)
        assert (_anchor_of(first, K) == n).all() and (_anchor_of(last, K) == n).all(), K
        if K % 4 == 0:                                                 # the vector path asks at multiples of 4 only
            assert (_anchor_of(last - 3, K) == n).all(), K
    for K in list(range(1, 129)) + [4093, 4095, 4096]:
        e = np.arange(256 * K, dtype=np.int64)
        assert (_anchor_of(e, K) == e // K).all(), K
    e = np.arange(256 * 4096, dtype=np.int64)
    assert (np.diff(_anchor_of(e, 4095)) >= 0).all()


# ---- the C entry points: workspace size and refusals (nothing below reaches a HIP call) --------------------------------------------------------
def test_workspace_bytes():
    from neuralnetworklibrary_amd._lib import lib
    for bs, A in ((1, 1), (1, 255), (1, 256), (1, 257), (2, 700), (17, 16385), (65535, 49104), (16, 49104)):
        assert lib.nnl_retina_loss_workspace_bytes(bs, A) == bs * rc.cdiv(A, 256) * 12
    for bs, A in ((0, 5), (5, 0), (-1, 5), (5, -1), (0, 0)):
        assert lib.nnl_retina_loss_workspace_bytes(bs, A) == 0


def _calls(lib, p):
    """(name, call(sizes, null=set of argument names, ws=..)) for the two entry points, every pointer the dummy address p unless named"""
    wsb = lambda bs, A: int(lib.nnl_retina_loss_workspace_bytes(bs, A))

    def fwd(bs, A, K, M, null=(), ws='ok'):
        a = {k: (None if k in null else p) for k in ('anchors', 'reg', 'clas', 'boxes', 'cats', 'state', 'npos', 'out')}
        need = wsb(bs, A)
        wsp, wsn = (None, need) if ws == 'null' else (p, need - 1) if ws == 'short' else (p, max(need, 1 << 20))
        return lib.nnl_retina_loss_fwd(a['anchors'], a['reg'], a['clas'], a['boxes'], a['cats'], a['state'], a['npos'], a['out'],
                                       bs, A, K, M, 0.5, 0.25, 2.0, wsp, wsn, None)

    def bwd(bs, A, K, M, null=(), ws='ok'):
        a = {k: (None if k in null else p) for k in ('anchors', 'reg', 'clas', 'boxes', 'cats', 'state', 'npos', 'grad_out', 'dreg', 'dclas')}
        return lib.nnl_retina_loss_bwd(a['anchors'], a['reg'], a['clas'], a['boxes'], a['cats'], a['state'], a['npos'], a['grad_out'],
                                       a['dreg'], a['dclas'], bs, A, K, M, 0.5, 0.25, 2.0, None)
    return (('retina_loss_fwd', fwd, ('anchors', 'reg', 'clas', 'state', 'npos', 'out')),
            ('retina_loss_bwd', bwd, ('anchors', 'reg', 'clas', 'state', 'npos', 'grad_out', 'dreg', 'dclas')))


def test_entry_points_refuse_bad_sizes_null_pointers_and_short_workspaces():
    from neuralnetworklibrary_amd._lib import lib
    INVALID, WORKSPACE = -1, -4
    one = torch.zeros(64, dtype=torch.float64)                         # any non-null host address: validation reads nothing
    p = one.data_ptr()
    ok = dict(bs=2, A=300, K=20, M=4)
    for name, call, required in _calls(lib, p):
        for key, bad in (('bs', 0), ('bs', 65536), ('bs', -1), ('A', 0), ('A', 1 << 30), ('K', 0), ('K', 4097), ('M', -1), ('M', 129)):
            sizes = dict(ok, **{key: bad})
            assert call(**sizes) == INVALID, '%s accepted %s' % (name, sizes)
            err = lib.nnl_last_error()
            assert name.encode() in err and (b'sizes' in err or b'at most 128 objects' in err), err
        for M in (0, 4):
            for arg in required:
                assert call(**dict(ok, M=M), null={arg}) == INVALID, '%s accepted %s = NULL' % (name, arg)
                assert name.encode() in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
        for arg in ('boxes', 'cats'):
            assert call(**ok, null={arg}) == INVALID, '%s accepted %s = NULL with M = 4' % (name, arg)
            assert name.encode() in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
            assert call(**dict(ok, M=128), null={arg}) == INVALID
    name, fwd, _ = _calls(lib, p)[0]
    for ws in ('null', 'short'):
        assert fwd(**ok, ws=ws) == WORKSPACE, 'workspace %s' % ws
        assert b'retina_loss_fwd' in lib.nnl_last_error() and b'workspace' in lib.nnl_last_error()
        assert fwd(1, 1, 1, 0, null={'boxes', 'cats'}, ws=ws) == WORKSPACE      # M = 0 with NULL boxes / cats passes the pointer checks
