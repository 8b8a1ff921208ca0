"""tests/detect_cases.py without a GPU: every regime of the detection-inference sweep has a case, every randn case meets its conditions on its
reference alone, a correct fp32 evaluation (restate32) passes every check the kernels will be judged by and sits inside HALF the box bound,
every mutant — a wrong NMS or decode written against the reference — fails on a case that the assertion names, and the C entry points refuse
what the header says they refuse, before any HIP call, so that runs here."""
import sys

import numpy as np
import pytest
import torch

import detect_cases as dc

f32, f64 = np.float32, np.float64
D_IDX, N_IDX = list(range(len(dc.DECODE_CASES))), list(range(len(dc.NMS_CASES)))
d_ids, n_ids = (lambda i: dc.DECODE_CASES[i].name), (lambda i: dc.NMS_CASES[i].name)


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
def test_census_every_regime_has_a_case():
    cov = dc.coverage()
    for k, names in cov.items():
        _say('DETECT_REGIME %-62s %s' % (k, ' '.join(names)))
    assert not [k for k, names in cov.items() if not names], 'regimes without a case: %s' % [k for k, v in cov.items() if not v]
    names = [c.name for c in dc.DECODE_CASES + dc.NMS_CASES]
    assert len(set(names)) == len(names)
    assert max(c.A for c in dc.DECODE_CASES) <= 2100 and max(c.top_k for c in dc.DECODE_CASES + dc.NMS_CASES) <= 300
    assert max(dc.nms_cand(c)['scores'].shape[1] for c in dc.NMS_CASES) <= 2100
    assert {c.mode for c in dc.DECODE_CASES} == {c.mode for c in dc.NMS_CASES} == {'grid', 'randn'}
    assert all(dc.ncase(n).null_order is False for n in dc.SHUFFLED) and dc.dcase(dc.WHOLE_WINDOW).window == (0.0, 0.0, dc.IMG, dc.IMG)


@pytest.mark.parametrize('i', D_IDX, ids=d_ids)
def test_decode_inputs_are_what_the_mode_promises(i):
    c = dc.DECODE_CASES[i]
    d, r = dc.decode_inputs(c), dc.decode_ref(c)
    assert all(d[k].dtype == f32 for k in ('anchors', 'reg', 'clas', 'mean', 'std'))
    assert d['anchors'].shape == (c.A, 4) and d['reg'].shape == (c.bs, c.A, 4) and d['clas'].shape == (c.bs, c.A, c.K)
    assert ((d['anchors'][:, 2] > d['anchors'][:, 0]) & (d['anchors'][:, 3] > d['anchors'][:, 1])).all() and np.isfinite(d['reg']).all()
    x0, y0, x1, y1 = dc.window_of(c)
    assert 0 <= x0 < x1 <= dc.IMG and 0 <= y0 < y1 <= dc.IMG
    for q in r:
        b = q['boxes']
        assert ((b[:, 0] >= x0) & (b[:, 1] >= y0) & (b[:, 2] <= x1) & (b[:, 3] <= y1) & (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])).all()
    if c.mode == 'grid':
        assert (d['anchors'] * 8 == np.round(d['anchors'] * 8)).all()
        dwh = d['reg'][:, :, 2:].astype(f64) * d['std'][2:].astype(f64) + d['mean'][2:].astype(f64)
        assert (dwh == 0).all(), 'dw = dh = 0 exactly'
        assert set(np.unique(d['clas'][~np.isnan(d['clas'])])) <= set(dc.GRID_SCORES)
        assert all(np.array_equal(q['boxes'].astype(f32).astype(f64), q['boxes']) and (q['boxes'] * 8 == np.round(q['boxes'] * 8)).all() for q in r)
    assert float(dc.ABOVE_THRESH) > float(dc.GRID_THRESH) and dc.ABOVE_THRESH - dc.GRID_THRESH == f32(2.0 ** -25)


@pytest.mark.parametrize('i', N_IDX, ids=n_ids)
def test_nms_inputs_are_valid(i):
    c = dc.NMS_CASES[i]
    cand = dc.nms_cand(c)
    bs, cap = cand['scores'].shape
    assert cand['boxes'].dtype == f32 and cand['scores'].dtype == f32 and cand['classes'].dtype == np.int32 and cand['count'].dtype == np.int32
    assert (cand['order'] is None) == c.null_order and 1 <= c.top_k <= 16384 and cap >= 1 and bs == len(c.images)
    for j in range(bs):
        n = min(int(cand['count'][j]), cap)
        assert cand['count'][j] >= 0 and np.isfinite(cand['boxes'][j, :n]).all() and np.isfinite(cand['scores'][j, :n]).all()
        if cand['order'] is not None:
            assert len(np.unique(cand['order'][j, :n])) == n, 'the order values of an image differ'
        if c.mode == 'grid':
            assert (cand['boxes'][j, :n] == np.round(cand['boxes'][j, :n])).all(), 'grid boxes lie on the integer grid'


# ---- the conditions of the randn cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [c for c in dc.DECODE_CASES + dc.NMS_CASES if c.mode == 'randn'], ids=lambda c: c.name)
def test_randn_cases_meet_their_conditions(c):
    dc.assert_conditions(c)
    _say('DETECT_SEED %s: attempt %d' % (c.name, (dc.decode_inputs(c) if isinstance(c, dc.DCase) else dc.nms_cand(c))['attempt']))


def test_condition_checks_notice_a_violation():
    c = dc.ncase('scan-rand-n257-k100')
    cand = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dc.nms_cand(c).items()}
    cand['scores'][0, 5] = cand['scores'][0, 9]
    assert any('share a score' in m for m in dc.nms_condition_failures(cand, c.top_k, c.max_overlap))
    two = dict(boxes=np.array([[[0, 0, 4, 4], [0, 0, 4, 2.0002]]], f32), classes=np.zeros((1, 2), np.int32), scores=np.array([[0.9, 0.8]], f32), order=None,
               count=np.array([2], np.int32))
    assert any('IoU within' in m for m in dc.nms_condition_failures(two, 2, 0.5))
    d = dc.dcase('r-a257-k1-bs3')
    x = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dc.decode_inputs(d).items()}
    x['clas'][0, 3, 0] = f32(d.thresh * (1 + 5e-7))
    assert any('thresh' in m for m in dc.decode_condition_failures(d, x))


# ---- a correct fp32 evaluation passes every check; the box bound -----------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize('i', D_IDX, ids=d_ids)
def test_fp32_restatement_of_the_decode_passes_within_half_the_bound(i):
    c = dc.DECODE_CASES[i]
    r = dc.decode_ref(c)
    q = dc.check_decode(c, r, dc.restate32(c))
    WORST[c.name] = q
    bound = max([float(x['bound'].max()) for x in r if len(x['order'])] or [0.0])
    _say('DETECT_FP32 %-20s candidates %s, err / bound %.3f, largest bound %.3e' % (c.name, [len(x['order']) for x in r], q, bound))
    assert q <= 0.5, 'the restatement must sit inside half the bound'
    assert bound <= 1e-5 * dc.IMG + 1e-5, 'no looser than test_bbox_inference.py grants at this scale'
    if len(WORST) == len(dc.DECODE_CASES):
        _say('DETECT_FP32 worst err / bound over the table: %.3f' % max(WORST.values()))


@pytest.mark.parametrize('i', D_IDX, ids=d_ids)
def test_fp32_restatement_of_decode_into_nms_passes(i):
    c = dc.DECODE_CASES[i]
    r = dc.decode_ref(c)
    cand = dc.decode_cand(c, r)
    nref = dc.nms_ref_of(cand, c.top_k, c.max_overlap)
    got = dc.restate32_decode(c)
    cand32 = dict(boxes=np.where(got['boxes'] == f32(dc.SENTINEL), f32(0), got['boxes']), classes=got['classes'], scores=got['scores'], order=got['order'],
                  count=got['count'])
    kept = dc.restate32_nms(cand32, c.top_k, c.max_overlap)
    dc.check_nms(c.name, nref, kept, boxes_exact=c.mode == 'grid')
    if c.mode == 'randn':
        assert dc.check_kept_boxes_within_bound(c, r, nref, kept) <= 0.5
    _say('DETECT_FP32 %-20s decode into NMS: kept %s of %s' % (c.name, list(nref['count']), list(cand['count'])))


@pytest.mark.parametrize('i', N_IDX, ids=n_ids)
def test_fp32_restatement_of_the_nms_passes(i):
    c = dc.NMS_CASES[i]
    cand, r = dc.nms_cand(c), dc.nms_ref(c)
    dc.check_nms(c.name, r, dc.restate32(c))
    _say('DETECT_FP32 %-24s kept %s of %s (top_k %d)' % (c.name, list(r['count']), list(cand['count']), c.top_k))
    if c.name in dc.SHUFFLED:
        dc.same_bits(r, dc.nms_ref_of(dc.shuffled(cand), c.top_k, c.max_overlap), c.name + ': the storage order must not matter to the reference')


@pytest.mark.parametrize('P', dc.MERGE_P)
def test_merge_reference_and_its_nms(P):
    m = dc.merge_inputs(P)
    cand = dc.merge_ref(m)
    assert cand['count'][1] == 0 and (cand['count'] == m['counts'].sum(1)).all() and cand['count'].max() > 64
    assert (cand['boxes'] * 2 == np.round(cand['boxes'] * 2)).all() and (cand['classes'][0, cand['count'][0]:] == -1).all()
    r = dc.nms_ref_of(cand, dc.MERGE_TOP_K, dc.MERGE_OVERLAP)
    dc.check_nms('merge P=%d' % P, r, dc.restate32_nms(cand, dc.MERGE_TOP_K, dc.MERGE_OVERLAP))
    assert r['count'][1] == 0 and 0 < r['count'][0] < min(cand['count'][0], dc.MERGE_TOP_K), 'some suppression, some survivors'
    assert (r['classes'][0, :r['count'][0]] >= 0).all(), 'a filler row is never kept'


def test_threshold_constructions_sit_exactly_on_the_thresholds():
    pair = np.array([[0, 0, 4, 4], [0, 0, 4, 2]], f32)
    assert dc._iou(pair, f32)[0, 1] == f32(0.5) and dc._iou(pair, f64)[0, 1] == 0.5
    assert float(dc.BELOW_HALF) < 0.5 and f32(0.5) - dc.BELOW_HALF == f32(2.0 ** -25)
    zero = np.array([[2, 2, 2, 3], [2, 2, 2, 3]], f32)
    assert np.isnan(dc._iou(zero, f32)[0, 1]) and np.isnan(dc._iou(zero, f64)[0, 1])
    ch = np.array(dc.CHAIN, f32)
    iou = dc._iou(ch, f64)
    assert iou[0, 1] > 0.5 and iou[1, 2] > 0.5 and iou[0, 2] < 0.5


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------------------
def _failing(check):
    out = []
    for name, run in check:
        try:
            run()
        except AssertionError:
            out.append(name)
    return out


@pytest.mark.parametrize('mutant', dc.NMS_MUTANTS)
def test_every_nms_mutant_fails_on_a_named_case(mutant):
    runs = [(c.name, (lambda c=c: dc.check_nms(c.name, dc.nms_ref(c), dc.nms_of(dc.nms_cand(c), c.top_k, c.max_overlap, f64, mutant)))) for c in dc.NMS_CASES]
    caught = _failing(runs)
    _say('DETECT_MUTANT %-18s caught by %s' % (mutant, ' '.join(caught)))
    expect = {'zombie': 'scan-chain-across-1', 'cross_class': 'scan-classes-m65', 'iou_ge': 'scan-iou-equal', 'tie_by_position': 'rank-n257-k100',
              'cut_after': 'scan-pairs-k100', 'no_carry': 'scan-chain-across-2'}[mutant]
    assert expect in caught, 'mutant %s passes the case built for it, %s (caught by: %s)' % (mutant, expect, caught)
    if mutant in ('zombie', 'no_carry', 'cross_class', 'cut_after'):
        assert any(n.startswith('scan-rand') for n in caught), 'mutant %s passes every randn case' % mutant
    if mutant == 'zombie':
        assert 'scan-chain-inside' in caught and 'scan-chain-across-2' in caught


@pytest.mark.parametrize('mutant', dc.DECODE_MUTANTS)
def test_every_decode_mutant_fails_on_a_named_case(mutant):
    runs = [(c.name, (lambda c=c: dc.check_decode(c, dc.decode_ref(c), dc.decode_as_returned(c, dc._decode(c, dc.decode_inputs(c), f64, mutant)))))
            for c in dc.DECODE_CASES]
    caught = _failing(runs)
    _say('DETECT_MUTANT %-18s caught by %s' % (mutant, ' '.join(caught)))
    expect = {'last_max': 'g-a256-k3-bs3', 'thresh_ge': 'g-a257-k4-edges', 'window_lo_ignored': 'g-a700-k2-window'}[mutant]
    assert expect in caught, 'mutant %s passes the case built for it, %s (caught by: %s)' % (mutant, expect, caught)
    if mutant == 'window_lo_ignored':
        assert 'r-a300-k7-window' in caught


def test_checkers_reject_damaged_results():
    c = dc.ncase('rank-n257-k100')
    r = dc.nms_ref(c)
    good = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    dc.check_nms(c.name, r, good)
    bad = dict(good, scores=good['scores'].copy()); bad['scores'][0, 99] = np.nextafter(bad['scores'][0, 99], f32(2))
    with pytest.raises(AssertionError, match='kept_scores'):
        dc.check_nms(c.name, r, bad)
    c2 = dc.ncase('rank-n1')
    r2 = dc.nms_ref(c2)
    bad = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in r2.items()}
    bad['classes'][0, 1] = 0                                           # a write past kept_count
    with pytest.raises(AssertionError, match='beyond its count'):
        dc.check_nms(c2.name, r2, bad)
    d = dc.dcase('r-a257-k1-bs3')
    ref = dc.decode_ref(d)
    got = dc.decode_as_returned(d, ref)
    assert dc.check_decode(d, ref, got) < 0.2                        # the fp64 boxes rounded to fp32: u |x| against a bound above 6 u |cx|
    bad = dict(got, boxes=got['boxes'].copy()); bad['boxes'][0, 0, 2] *= f32(1 + 4e-6)
    with pytest.raises(AssertionError, match='err / bound'):
        dc.check_decode(d, ref, bad)
    bad = dict(got, count=got['count'].copy()); bad['count'][1] = 1
    with pytest.raises(AssertionError, match='cand_count'):
        dc.check_decode(d, ref, bad)


# ---- the C entry points: workspace size and refusals (nothing below reaches a HIP call) --------------------------------------------------------
def _ws_bytes(bs, top_k):
    return bs * top_k * 24 + bs * 16 + bs * top_k * dc.cdiv(top_k, 64) * 8


def test_nms_workspace_bytes():
    from neuralnetworklibrary_amd._lib import lib
    for bs, k in ((1, 1), (1, 63), (1, 64), (1, 65), (3, 200), (16, 1000), (2, 16384), (65535, 100)):
        assert lib.nnl_nms_workspace_bytes(bs, k) == _ws_bytes(bs, k)
    for bs, k in ((0, 5), (5, 0), (-1, 5), (5, -1), (0, 0)):
        assert lib.nnl_nms_workspace_bytes(bs, k) == 0


def test_detect_entry_points_reject_bad_arguments_before_any_hip_call():
    from neuralnetworklibrary_amd._lib import lib
    INVALID, WORKSPACE = -1, -4
    host = torch.zeros(64, dtype=torch.float64)                        # any non-null host address: validation reads nothing
    p = host.data_ptr()
    dec_ptrs = ('anchors', 'reg', 'clas', 'mean4', 'std4', 'cand_boxes', 'cand_classes', 'cand_scores', 'cand_order', 'cand_count')

    def decode(bs=2, A=300, K=3, null=(), window=None):
        a = {k: (None if k in null else p) for k in dec_ptrs}
        head = (a['anchors'], a['reg'], a['clas'], bs, A, K, a['mean4'], a['std4'], 0.05)
        tail = (a['cand_boxes'], a['cand_classes'], a['cand_scores'], a['cand_order'], a['cand_count'], None)
        if window is None:
            return lib.nnl_bbox_decode(*head, 128.0, 128.0, *tail)
        return lib.nnl_bbox_decode_window(*head, *window, *tail)

    for window in (None, (8.0, 8.0, 100.0, 100.0)):
        for arg in dec_ptrs:
            assert decode(null={arg}, window=window) == INVALID, 'bbox_decode accepted %s = NULL' % arg
            assert b'bbox_decode' in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
        for key, bad in (('bs', 0), ('bs', -1), ('bs', 65536), ('A', 0), ('A', -5), ('A', 1 << 30), ('K', 0), ('K', -1)):
            assert decode(**{key: bad}, window=window) == INVALID, 'bbox_decode accepted %s = %d' % (key, bad)
            assert b'bbox_decode' in lib.nnl_last_error() and b'sizes' in lib.nnl_last_error()
    for window in ((-1.0, 0.0, 10.0, 10.0), (0.0, -1.0, 10.0, 10.0), (10.0, 0.0, 10.0, 10.0), (0.0, 10.0, 10.0, 10.0), (12.0, 0.0, 10.0, 10.0),
                   (float('nan'), 0.0, 10.0, 10.0), (0.0, 0.0, float('nan'), 10.0), (0.0, 0.0, 10.0, float('nan'))):
        assert decode(window=window) == INVALID, 'bbox_decode_window accepted the window %s' % (window,)
        assert b'bbox_decode_window' in lib.nnl_last_error() and b'window' in lib.nnl_last_error()

    nms_ptrs = ('cand_boxes', 'cand_classes', 'cand_scores', 'cand_order', 'cand_count', 'kept_boxes', 'kept_classes', 'kept_scores', 'kept_count')

    def nms(bs=2, cap=300, top_k=100, null=(), ws='ok'):
        a = {k: (None if k in null else p) for k in nms_ptrs}
        need = _ws_bytes(bs, top_k) if bs > 0 and top_k > 0 else 0
        wsp, wsn = (None, need) if ws == 'null' else (p, need - 1) if ws == 'short' else (p, need)
        return lib.nnl_nms(a['cand_boxes'], a['cand_classes'], a['cand_scores'], a['cand_order'], a['cand_count'], bs, cap, top_k, 0.5, a['kept_boxes'],
                           a['kept_classes'], a['kept_scores'], a['kept_count'], wsp, wsn, None)

    for arg in nms_ptrs:
        if arg != 'cand_order':                                        # cand_order may be NULL
            assert nms(null={arg}) == INVALID, 'nms accepted %s = NULL' % arg
            assert b'nms' in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
    for key, bad in (('bs', 0), ('bs', -1), ('bs', 65536), ('cap', 0), ('cap', -1), ('cap', 1 << 30), ('top_k', 0), ('top_k', -1), ('top_k', 16385)):
        assert nms(**{key: bad}) == INVALID, 'nms accepted %s = %d' % (key, bad)
        assert b'nms' in lib.nnl_last_error() and b'sizes' in lib.nnl_last_error()
    for ws in ('null', 'short'):
        assert nms(ws=ws) == WORKSPACE, 'workspace %s' % ws
        assert b'nms' in lib.nnl_last_error() and b'workspace' in lib.nnl_last_error()
        assert nms(null={'cand_order'}, ws=ws) == WORKSPACE            # a NULL cand_order passes the pointer check
        assert nms(top_k=16384, ws=ws) == WORKSPACE

    mrg_ptrs = ('boxes', 'classes', 'scores', 'counts', 'undo', 'cand_boxes', 'cand_classes', 'cand_scores', 'cand_order', 'cand_count')

    def merge(L=2, P=4, M=5, null=()):
        a = {k: (None if k in null else p) for k in mrg_ptrs}
        return lib.nnl_tta_bbox_merge(a['boxes'], a['classes'], a['scores'], a['counts'], a['undo'], L, P, M, a['cand_boxes'], a['cand_classes'],
                                      a['cand_scores'], a['cand_order'], a['cand_count'], None, None)

    for arg in mrg_ptrs:
        assert merge(null={arg}) == INVALID and b'tta_bbox_merge' in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
    for key, bad in (('L', 0), ('L', 1 << 31), ('P', 0), ('P', 65), ('M', 0), ('M', (1 << 20) + 1)):
        assert merge(**{key: bad}) == INVALID and b'sizes' in lib.nnl_last_error(), 'tta_bbox_merge accepted %s = %d' % (key, bad)
    assert merge(P=64, M=(1 << 14) + 1) == INVALID, 'P M above 2^20'
