"""The detection-inference C ABI (nnl_bbox_decode, nnl_bbox_decode_window, nnl_nms, nnl_tta_bbox_merge; include/nnl.h, csrc/detect.hip) called
directly over the cases of tests/detect_cases.py, against their references.

Every output sits between guard bands and is pre-filled with a sentinel: afterwards the bands are intact and every slot at or beyond cand_count /
kept_count still holds the sentinel (the merge kernel's documented fillers are asserted instead).  Decode: cand_count exactly, then the
candidates sorted by cand_order — anchors, classes and scores exactly, boxes bit for bit (grid) or within the derived bound (randn).  nnl_nms:
kept boxes, classes, scores and count bit for bit; a second run bitwise equal; a run on a workspace of exactly nnl_nms_workspace_bytes filled
with 0xFF bytes and one on a zeroed workspace bitwise equal (the mask tiles and words that are never written are never read); the same
candidates in another storage order give the same bits.  Then decode into NMS end to end in both modes, the merge kernel's output (fillers
included) straight into nnl_nms, and the Python callers nms() and BBoxPredictor.survivors_on_device() at top_k above the candidate count, an
empty input and a batch with an empty image.  The randn conditions are re-asserted before a kernel is judged.  Every shape is inside the
entry points' stated domain: no test provokes a fault.

The file takes under 2 s on an MI355X (54 tests in 1.7 s; the slowest are the first ones to load the library and the Python callers, 0.6 s and
0.3 s; every other test 0.1 s or less).
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import detect_cases as dc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                                     # elements (bytes for the workspace) of guard band on either side of a buffer
BANDS = {torch.uint8: 0xA5, torch.int32: 0x3C3C3C3C, torch.float32: -54321.0}
D_IDX, N_IDX = list(range(len(dc.DECODE_CASES))), list(range(len(dc.NMS_CASES)))
d_ids, n_ids = (lambda i: dc.DECODE_CASES[i].name), (lambda i: dc.NMS_CASES[i].name)
f32 = np.float32


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


class Guarded:
    """`shape` elements inside a larger allocation with guard bands on both sides, pre-filled with `fill`"""

    def __init__(self, shape, dtype, fill):
        self.shape, self.numel, self.band = shape, int(np.prod(shape)), BANDS[dtype]
        self.buf = torch.full((self.numel + 2 * GUARD,), self.band, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.numel]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:GUARD] == self.band).all()) and bool((self.buf[GUARD + self.numel:] == self.band).all())

    def numpy(self):
        return self.t.view(self.shape).cpu().numpy()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)        # a copy: the shared inputs are read-only


def _collect(bufs, what):
    torch.cuda.synchronize()
    for k, g in bufs.items():
        assert g.intact(), '%s wrote outside %s (guard band touched)' % (what, k)
    return {k: g.numpy() for k, g in bufs.items()}


def run_decode(lib, c, d, window='case'):
    """nnl_bbox_decode, or nnl_bbox_decode_window when the case (or `window`) has one; the outputs as numpy arrays"""
    window = c.window if window == 'case' else window
    x = {k: dev(d[k]) for k in ('anchors', 'reg', 'clas')}
    bufs = dict(boxes=Guarded((c.bs, c.A, 4), torch.float32, dc.SENTINEL), classes=Guarded((c.bs, c.A), torch.int32, dc.INT_SENTINEL),
                scores=Guarded((c.bs, c.A), torch.float32, dc.SENTINEL), order=Guarded((c.bs, c.A), torch.int32, dc.INT_SENTINEL),
                count=Guarded((c.bs,), torch.int32, dc.INT_SENTINEL))
    mean, std = np.ascontiguousarray(d['mean']), np.ascontiguousarray(d['std'])
    head = (ptr(x['anchors']), ptr(x['reg']), ptr(x['clas']), c.bs, c.A, c.K, mean.ctypes.data, std.ctypes.data, c.thresh)
    tail = (ptr(bufs['boxes'].t), ptr(bufs['classes'].t), ptr(bufs['scores'].t), ptr(bufs['order'].t), ptr(bufs['count'].t), None)
    if window is None:
        st = lib.nnl_bbox_decode(*head, dc.IMG, dc.IMG, *tail)
    else:
        st = lib.nnl_bbox_decode_window(*head, *window, *tail)
    assert st == 0, 'nnl_bbox_decode: %d %s' % (st, lib.nnl_last_error())
    got = _collect(bufs, c.name + ': nnl_bbox_decode')
    for k in x:
        assert np.array_equal(x[k].cpu().numpy().view(np.int32), np.ascontiguousarray(d[k]).view(np.int32)), '%s: the decode wrote to its input %s' % (c.name, k)
    return got


def run_nms(lib, name, cand, top_k, thr, ws_fill=0xFF, on_device=None):
    """nnl_nms on a workspace of exactly nnl_nms_workspace_bytes, pre-filled with ws_fill bytes; cand: numpy arrays, or device tensors
    in on_device (the output of another kernel)"""
    x = on_device if on_device is not None else {k: dev(cand[k]) for k in ('boxes', 'classes', 'scores', 'order', 'count')}
    bs, cap = x['scores'].shape
    wsb = int(lib.nnl_nms_workspace_bytes(bs, top_k))
    assert wsb == bs * top_k * 24 + bs * 16 + bs * top_k * dc.cdiv(top_k, 64) * 8
    ws = Guarded((wsb,), torch.uint8, ws_fill)
    bufs = dict(boxes=Guarded((bs, top_k, 4), torch.float32, dc.SENTINEL), classes=Guarded((bs, top_k), torch.int32, dc.INT_SENTINEL),
                scores=Guarded((bs, top_k), torch.float32, dc.SENTINEL), count=Guarded((bs,), torch.int32, dc.INT_SENTINEL))
    st = lib.nnl_nms(ptr(x['boxes']), ptr(x['classes']), ptr(x['scores']), ptr(x['order']), ptr(x['count']), bs, cap, top_k, thr, ptr(bufs['boxes'].t),
                     ptr(bufs['classes'].t), ptr(bufs['scores'].t), ptr(bufs['count'].t), ptr(ws.t), wsb, None)
    assert st == 0, 'nnl_nms: %d %s' % (st, lib.nnl_last_error())
    got = _collect(bufs, name + ': nnl_nms')
    assert ws.intact(), '%s: nnl_nms wrote outside its workspace of %d bytes' % (name, wsb)
    if on_device is None:
        for k in ('boxes', 'classes', 'scores', 'order', 'count'):
            if cand[k] is not None:
                assert np.array_equal(x[k].cpu().numpy().view(np.int32), np.ascontiguousarray(cand[k]).view(np.int32)), '%s: nnl_nms wrote to its input %s' % (name, k)
    return got


def sorted_by_order(got):
    """the candidates of every image sorted by cand_order (the append order is not defined), the rest of each row as it is"""
    out = {k: v.copy() for k, v in got.items()}
    for i, n in enumerate(got['count']):
        p = np.argsort(got['order'][i, :n], kind='stable')
        for k in ('boxes', 'classes', 'scores', 'order'):
            out[k][i, :n] = got[k][i, :n][p]
    return out


# ---- decode ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', D_IDX, ids=d_ids)
def test_decode_abi_case_by_case_vs_fp64(i):
    from neuralnetworklibrary_amd._lib import lib
    c = dc.DECODE_CASES[i]
    dc.assert_conditions(c)
    d, r = dc.decode_inputs(c), dc.decode_ref(c)
    got = run_decode(lib, c, d)
    _say('DETECT_ABI %s cand_count %s reference %s' % (c.name, got['count'], [len(q['order']) for q in r]))
    q = dc.check_decode(c, r, got)
    _say('DETECT_ABI %s decode err / bound %.3f' % (c.name, q))
    a, b = sorted_by_order(got), sorted_by_order(run_decode(lib, c, d))
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), '%s: two runs on the same inputs differ in %s (after sorting by cand_order)' % (c.name, k)


def test_a_window_equal_to_the_image_is_the_plain_decode_bit_for_bit():
    from neuralnetworklibrary_amd._lib import lib
    c = dc.dcase(dc.WHOLE_WINDOW)
    d = dc.decode_inputs(c)
    a, b = sorted_by_order(run_decode(lib, c, d)), sorted_by_order(run_decode(lib, c, d, window=None))
    assert a['count'][0] > 256
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), '%s: nnl_bbox_decode_window on the whole image and nnl_bbox_decode differ in %s' % (c.name, k)


# ---- rank-sort, mask and scan -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', N_IDX, ids=n_ids)
def test_nms_abi_case_by_case_vs_fp64(i):
    from neuralnetworklibrary_amd._lib import lib
    c = dc.NMS_CASES[i]
    dc.assert_conditions(c)
    cand, r = dc.nms_cand(c), dc.nms_ref(c)
    got = run_nms(lib, c.name, cand, c.top_k, c.max_overlap, ws_fill=0xFF)
    _say('DETECT_ABI %s kept_count %s reference %s' % (c.name, got['count'], r['count']))
    dc.check_nms(c.name, r, got)
    dc.same_bits(got, run_nms(lib, c.name, cand, c.top_k, c.max_overlap, ws_fill=0xFF), c.name + ': two runs on the same inputs')
    dc.same_bits(got, run_nms(lib, c.name, cand, c.top_k, c.max_overlap, ws_fill=0x00), c.name + ': workspace of 0xFF bytes against a zeroed one')


@pytest.mark.parametrize('name', dc.SHUFFLED)
def test_the_storage_order_of_the_candidates_changes_no_bit(name):
    """the claim of detect.hip's header: the atomic append order of the decode does not matter to what nnl_nms returns"""
    from neuralnetworklibrary_amd._lib import lib
    c = dc.ncase(name)
    cand = dc.nms_cand(c)
    other = dc.shuffled(cand)
    assert not np.array_equal(other['order'], cand['order'])
    a, b = run_nms(lib, name, cand, c.top_k, c.max_overlap), run_nms(lib, name, other, c.top_k, c.max_overlap)
    dc.same_bits(a, b, name + ': the same candidates in two storage orders')
    dc.check_nms(name, dc.nms_ref(c), b)


# ---- decode into NMS, end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', D_IDX, ids=d_ids)
def test_decode_into_nms_end_to_end(i):
    """the kernel's own candidates, in the order its atomics left them, into nnl_nms with cap = A"""
    from neuralnetworklibrary_amd._lib import lib
    c = dc.DECODE_CASES[i]
    dc.assert_conditions(c)
    d, r = dc.decode_inputs(c), dc.decode_ref(c)
    nref = dc.nms_ref_of(dc.decode_cand(c, r), c.top_k, c.max_overlap)
    got = run_decode(lib, c, d)
    dc.check_decode(c, r, got)
    kept = run_nms(lib, c.name, got, c.top_k, c.max_overlap)
    _say('DETECT_ABI %s end to end kept_count %s reference %s' % (c.name, kept['count'], nref['count']))
    dc.check_nms(c.name + ' (decode into NMS)', nref, kept, boxes_exact=c.mode == 'grid')
    if c.mode == 'randn':
        _say('DETECT_ABI %s end to end kept boxes err / bound %.3f' % (c.name, dc.check_kept_boxes_within_bound(c, r, nref, kept)))


# ---- the merge kernel's output, fillers included, straight into nnl_nms ----------------------------------------------------------------------------------
@pytest.mark.parametrize('P', dc.MERGE_P)
def test_merge_into_nms(P):
    from neuralnetworklibrary_amd._lib import lib
    m = dc.merge_inputs(P)
    L, M, cap = m['L'], m['M'], P * m['M']
    want = dc.merge_ref(m)
    x = {k: dev(m[k]) for k in ('boxes', 'classes', 'scores', 'counts')}
    undo = dev(np.ascontiguousarray(m['undo']).view(np.uint8).reshape(L, P, dc.UNDO.itemsize))
    bufs = dict(boxes=Guarded((L, cap, 4), torch.float32, dc.SENTINEL), classes=Guarded((L, cap), torch.int32, dc.INT_SENTINEL),
                scores=Guarded((L, cap), torch.float32, dc.SENTINEL), order=Guarded((L, cap), torch.int32, dc.INT_SENTINEL),
                count=Guarded((L,), torch.int32, dc.INT_SENTINEL))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = lib.nnl_tta_bbox_merge(ptr(x['boxes']), ptr(x['classes']), ptr(x['scores']), ptr(x['counts']), ptr(undo), L, P, M, ptr(bufs['boxes'].t),
                                ptr(bufs['classes'].t), ptr(bufs['scores'].t), ptr(bufs['order'].t), ptr(bufs['count'].t), ptr(flag), None)
    assert st == 0, 'nnl_tta_bbox_merge: %d %s' % (st, lib.nnl_last_error())
    got = _collect(bufs, 'merge P=%d' % P)
    assert int(flag.item()) == 0
    for k in ('count', 'boxes', 'classes', 'scores', 'order'):                  # the fillers are part of `want`: box 0, class -1, score 0, order = position
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), 'merge P=%d: cand_%s differs from the numpy restatement (fillers included)' % (P, k)
    nref = dc.nms_ref_of(want, dc.MERGE_TOP_K, dc.MERGE_OVERLAP)
    on_device = {k: bufs[k].t.view(bufs[k].shape) for k in bufs}
    kept = run_nms(lib, 'merge P=%d' % P, None, dc.MERGE_TOP_K, dc.MERGE_OVERLAP, on_device=on_device)
    _say('DETECT_ABI merge P=%d cand_count %s kept_count %s' % (P, got['count'], kept['count']))
    dc.check_nms('merge P=%d into NMS' % P, nref, kept)
    dc.same_bits(kept, run_nms(lib, 'merge P=%d' % P, None, dc.MERGE_TOP_K, dc.MERGE_OVERLAP, ws_fill=0, on_device=on_device), 'merge into NMS, zeroed workspace')


# ---- the Python callers --------------------------------------------------------------------------------------------------------------------------------
def test_nms_wrapper_with_top_k_above_the_count_and_an_empty_input():
    from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import nms
    c = dc.ncase('scan-rand-n257-k100')
    cand = dc.nms_cand(c)
    n = int(cand['count'][0])
    r = dc.nms_ref_of({k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in cand.items()}, 1000, c.max_overlap)
    # nms() takes no order: the position is the order, and the scores of a randn case differ, so the order decides nothing
    B, C, S = nms(dev(cand['boxes'][0, :n]), dev(cand['classes'][0, :n]).long(), dev(cand['scores'][0, :n]), max_overlap=c.max_overlap, top_k=1000, max_boxes=10 ** 6)
    k = int(r['count'][0])
    assert 0 < k < n and len(B) == len(C) == len(S) == k
    assert np.array_equal(np.array(B, f32).view(np.int32), r['boxes'][0, :k].view(np.int32)) and np.array_equal(np.array(S, f32).view(np.int32), r['scores'][0, :k].view(np.int32))
    assert [int(v) for v in C] == [int(v) for v in r['classes'][0, :k]]
    empty = torch.zeros(0, 4, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV), torch.zeros(0, device=DEV)
    assert nms(*empty) == ([], [], [])
    B, C, S = nms(dev(cand['boxes'][1, :1]), dev(cand['classes'][1, :1]).long(), dev(cand['scores'][1, :1]), top_k=1000)
    assert len(B) == 1 and np.array_equal(np.array(B[0], f32), cand['boxes'][1, 0]) and int(C[0]) == cand['classes'][1, 0] and f32(S[0]) == cand['scores'][1, 0]


@pytest.mark.parametrize('name', ['g-a256-k3-bs3', 'r-a257-k1-bs3'])
def test_survivors_on_device_with_an_empty_image_and_top_k_above_the_anchors(name):
    from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import BBoxPredictor
    c = dc.dcase(name)
    dc.assert_conditions(c)
    d, r = dc.decode_inputs(c), dc.decode_ref(c)
    assert any(len(q['order']) == 0 for q in r) and c.bs >= 3
    pred = BBoxPredictor(mean=list(d['mean']), std=list(d['std']))
    img = torch.zeros(c.bs, 3, int(dc.IMG), int(dc.IMG), device=DEV)
    for top_k in (c.top_k, 1000):                                      # 1000 > A: the wrapper cuts top_k to the anchor count
        nref = dc.nms_ref_of(dc.decode_cand(c, r), min(top_k, c.A), c.max_overlap)
        kb, kc, ks, kn = pred.survivors_on_device(img, dev(d['reg']), dev(d['clas']), dev(d['anchors']), thresh=c.thresh, max_overlap=c.max_overlap, top_k=top_k)
        assert tuple(kb.shape) == (c.bs, min(top_k, c.A), 4) and kn.dtype == torch.int32
        n = kn.cpu().numpy()
        assert np.array_equal(n, nref['count']), '%s top_k %d: kept_count %s, reference %s' % (name, top_k, n, nref['count'])
        kept = dict(boxes=np.full(nref['boxes'].shape, dc.SENTINEL, f32), classes=np.full(nref['classes'].shape, dc.INT_SENTINEL, np.int32),
                    scores=np.full(nref['scores'].shape, dc.SENTINEL, f32), count=n)
        for i in range(c.bs):                                          # torch.empty outputs: only the slots below kept_count mean anything
            kept['boxes'][i, :n[i]], kept['classes'][i, :n[i]], kept['scores'][i, :n[i]] = kb[i, :n[i]].cpu().numpy(), kc[i, :n[i]].cpu().numpy(), ks[i, :n[i]].cpu().numpy()
        dc.check_nms('%s through survivors_on_device, top_k %d' % (name, top_k), nref, kept, boxes_exact=c.mode == 'grid')
        if c.mode == 'randn':
            dc.check_kept_boxes_within_bound(c, r, nref, kept)
    P, C, S = pred(img, dev(d['reg']), dev(d['clas']), dev(d['anchors']), thresh=c.thresh, max_overlap=c.max_overlap, top_k=1000, max_boxes=10 ** 6)
    assert [len(b) for b in P] == list(nref['count']) and P[1] == [] and C[1] == [] and S[1] == []
