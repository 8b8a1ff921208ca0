"""Detection evaluation (K14): the COCO / Pascal protocol (ImageLearner.coco_pascal_eval, ops.det_eval_coco) and the mean average
precision on the device (mAP_device, ops.det_map), against golden G23 (tools/gen_golden_det_eval.py: the real reference's COCOeval,
with the tool's restatement of pycocotools' box IoU, and the real reference's mAP1 / mAP).
CPU: a numpy restatement of the four kernel jobs, structured as the kernels are (per group, per (area range, threshold) lane, per
(category, area, maxDets, threshold) curve), is pinned to G23; ops.det_eval_pack's layout; every ValueError; the C entries' argument
validation.  GPU: the kernels against G23 and the restatement, exactly where every quantity is an integer count or a single IEEE fp64
operation on identical inputs in identical order (the COCO protocol, the mAP flags), and within L 2^-52 relative where only the
summation order of L non-negative terms differs (the mAP values)."""
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gen_golden_det_eval as GEN  # noqa: E402

S = GEN.SETTINGS
EPS = 2.0 ** -52


# ---- the shared reference data: computed once, never changed ----------------------------------------------------------------

class _Data:
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from neuralnetworklibrary_amd import ops
            d = types.SimpleNamespace()
            d.G = load_golden('g23_det_eval')
            d.coco, d.ids, d.preds, d.cat2dscat, d.categories = GEN.build()
            d.targets = GEN.targets_of(d.coco, d.ids, d.cat2dscat)
            d.packed = ops.det_eval_pack(d.preds, coco=d.coco, image_ids=d.ids, cat2dscat=d.cat2dscat, max_det=S['maxDets'][-1])
            d.mpacked = ops.det_eval_pack(d.preds, targets=d.targets, n_categories=len(d.categories))
            d.thr, d.rng = np.asarray(S['iouThrs'], dtype=np.float64), np.asarray(S['areaRng'], dtype=np.float64)
            d.r_match = r_coco_match(d.packed, d.thr, d.rng)
            d.r_acc = r_coco_accumulate(d.packed, *d.r_match[:3], S['recThrs'], S['maxDets'])
            d.r_flags = r_map_match(d.mpacked, S['mAP_thresholds'])
            d.r_map = r_map_integrate(d.mpacked, d.r_flags)
            cls._made = d
        return cls._made


# ---- numpy restatement of the kernels ---------------------------------------------------------------------------------------

def r_overlap(D, G, crowd):
    "job a's overlap of one detection and one ground truth, [x, y, w, h] in fp64, one operation at a time"
    w = min(D[0] + D[2], G[0] + G[2]) - max(D[0], G[0])
    h = min(D[1] + D[3], G[1] + G[3]) - max(D[1], G[1])
    if w <= 0 or h <= 0:
        return 0.0
    inter, da = w * h, D[2] * D[3]
    return inter / (da if crowd else da + G[2] * G[3] - inter)


def r_match_group(dt_box, gt_box, gt_area, gt_flags, thr, rng):
    "one group (one wave): the overlap matrix once, then one lane per (area range, threshold)"
    D, G, T, A = len(dt_box), len(gt_box), len(thr), len(rng)
    iou = np.array([[r_overlap(dt_box[d], gt_box[j], gt_flags[j] & 1) for j in range(G)] for d in range(D)], dtype=np.float64).reshape(D, G)
    ig = np.array([[bool(gt_flags[j] & 2) or gt_area[j] < rng[a, 0] or gt_area[j] > rng[a, 1] for j in range(G)] for a in range(A)], dtype=bool).reshape(A, G)
    dtm, dtig = np.zeros((A, T, D), np.int32), np.zeros((A, T, D), np.uint8)
    for lane in range(A * T):
        a, t = divmod(lane, T)
        taken = np.zeros(G, bool)
        for d in range(D):
            bar, m, m_ig = min(thr[t], 1 - 1e-10), -1, 0
            for phase in (0, 1):                                             # the counting ground truths first, then the ignored
                if phase == 1 and m > -1 and m_ig == 0:
                    break
                for j in range(G):
                    if ig[a, j] != phase or (taken[j] and not gt_flags[j] & 1) or iou[d, j] < bar:
                        continue
                    bar, m, m_ig = iou[d, j], j, phase
            if m >= 0:
                taken[m], dtm[a, t, d], dtig[a, t, d] = True, m + 1, m_ig
            else:
                area = dt_box[d, 2] * dt_box[d, 3]
                dtig[a, t, d] = area < rng[a, 0] or area > rng[a, 1]
    gtig_sorted = np.stack([np.sort(ig[a].astype(np.uint8), kind='stable') for a in range(A)]).reshape(A, G)
    return dtm, dtig, (~ig).sum(axis=1).astype(np.int32), gtig_sorted


def r_coco_match(p, thr, rng):
    NG, A, T = len(p['grp_cat']), len(rng), len(thr)
    dtm, dtig = np.zeros((A, T, len(p['dt_score'])), np.int32), np.zeros((A, T, len(p['dt_score'])), np.uint8)
    npig, gtig = np.zeros((A, NG), np.int32), np.zeros((A, len(p['gt_area'])), np.uint8)
    for g in range(NG):
        d0, d1, q0, q1 = p['dt_off'][g], p['dt_off'][g + 1], p['gt_off'][g], p['gt_off'][g + 1]
        dtm[:, :, d0:d1], dtig[:, :, d0:d1], npig[:, g], gtig[:, q0:q1] = r_match_group(
            p['dt_box'][d0:d1], p['gt_box'][q0:q1], p['gt_area'][q0:q1], p['gt_flags'][q0:q1], thr, rng)
    return dtm, dtig, npig, gtig


def r_coco_accumulate(p, dtm, dtig, npig, recThrs, maxDets):
    "job b: one curve per (k, a, m, t) over the category's detections in score order; the positions where the recall reaches each threshold"
    rec = np.asarray(recThrs, dtype=np.float64)
    A, T, _ = dtm.shape
    K, M, R = p['K'], len(maxDets), len(rec)
    precision, scores, recall = -np.ones((T, R, K, A, M)), -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        g0, g1 = p['cat_grp_off'][k], p['cat_grp_off'][k + 1]
        order = p['order'][p['cat_dt_off'][k]:p['cat_dt_off'][k + 1]]
        for a in range(A):
            n_pig = int(npig[a, g0:g1].sum())
            if g0 == g1 or n_pig == 0:
                continue
            for m in range(M):
                kept = order[p['dt_rank'][order] < maxDets[m]]
                for t in range(T):
                    tp = np.cumsum((dtm[a, t, kept] != 0) & (dtig[a, t, kept] == 0)).astype(np.float64)
                    fp = np.cumsum((dtm[a, t, kept] == 0) & (dtig[a, t, kept] == 0)).astype(np.float64)
                    rc, pr = tp / n_pig, tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if len(kept) else 0.0
                    right = np.maximum.accumulate(pr[::-1])[::-1]
                    for r in range(R):
                        reached = np.nonzero(rc >= rec[r])[0]
                        at = reached[0] if len(reached) else -1
                        precision[t, r, k, a, m] = right[at] if at >= 0 else 0.0
                        scores[t, r, k, a, m] = p['dt_score'][kept[at]] if at >= 0 else 0.0
    return precision, recall, scores


def r_jaccard(t, b):
    "retinanet.jaccard for one (ground truth, prediction) pair of float32 min-max boxes, in its operation order"
    f = np.float32
    a1, a2 = f(f(t[2] - t[0]) * f(t[3] - t[1])), f(f(b[2] - b[0]) * f(b[3] - b[1]))
    iw = max(f(min(t[2], b[2]) - max(t[0], b[0])), f(0))
    ih = max(f(min(t[3], b[3]) - max(t[1], b[1])), f(0))
    inter = f(iw * ih)
    with np.errstate(all='ignore'):
        return f(inter / f(f(a1 + a2) - inter))


def r_map_match(p, thresholds):
    "job c: per group, every ground truth marks its first arg-max prediction where the overlap is strictly above the threshold"
    correct = np.zeros((len(thresholds), len(p['pr_score'])), np.uint8)
    for g in range(len(p['grp_cat'])):
        p0, p1, q0, q1 = p['pr_off'][g], p['pr_off'][g + 1], p['gt_off'][g], p['gt_off'][g + 1]
        if p0 == p1:
            continue
        for j in range(q0, q1):
            jac = np.array([r_jaccard(p['gt_box'][j], p['pr_box'][i]) for i in range(p0, p1)], dtype=np.float32)
            best = int(jac.argmax())
            for t, thr in enumerate(thresholds):
                if jac[best] > thr:
                    correct[t, p0 + best] = 1
    return correct


def r_map_integrate(p, correct):
    "job d: one curve per (category, threshold); inside a run of equal scores the correct predictions come first"
    T, C = len(correct), p['C']
    out = np.zeros((T, C))
    for c in range(C):
        order = p['order'][p['cat_pr_off'][c]:p['cat_pr_off'][c + 1]]
        sc = p['pr_score'][order]
        for t in range(T):
            ok = correct[t, order]
            v, seen, head, before = np.zeros(len(order)), 0, 0, 0
            for i in range(len(order)):
                if i == 0 or sc[i] != sc[i - 1]:
                    head, before = i, seen
                if ok[i]:
                    seen += 1
                    v[i] = seen * (1.0 / (head + seen - before))
            right = np.maximum.accumulate(v[::-1])[::-1] if len(v) else v
            total = 0.0
            for i in np.nonzero(ok)[0]:
                total += right[i]
            with np.errstate(all='ignore'):
                out[t, c] = np.float64(total) / np.float64(p['ntrue'][c])
    return out


def host_map1(preds, targets, C, thresholds):
    "[T, C] of the host path's V.mAP1 and the prediction count L of each category"
    from neuralnetworklibrary_amd.Applications import Vision as V
    N = len(preds)
    targs, pp, ss = ([[[] for _ in range(N)] for _ in range(C)] for _ in range(3))
    for i in range(N):
        for j in range(len(preds[i][0])):
            pp[preds[i][1][j]][i].append(preds[i][0][j])
            ss[preds[i][1][j]][i].append(preds[i][2][j])
        for b, c in targets[i]:
            targs[c][i].append(b)
    with np.errstate(all='ignore'):
        vals = np.array([[V.mAP1(targs[c], pp[c], ss[c], t) for c in range(C)] for t in thresholds])
    return vals, np.array([sum(len(x) for x in pp[c]) for c in range(C)])


def random_set(seed, n_images, n_cats, per_image, levels):
    "a larger random set for the tile edges: (coco dict, ids, predictions, cat2dscat)"
    rs = np.random.RandomState(seed)
    ids = [int(v) + 1 for v in rs.permutation(n_images)]
    coco = {'images': [{'id': i} for i in ids], 'categories': [{'id': 10 + c} for c in range(n_cats)], 'annotations': []}
    preds = []
    for i in range(n_images):
        B, Cl, Sc = [], [], []
        for c in range(n_cats):
            for _ in range(rs.randint(0, 4)):
                x, y, w, h = (np.round(rs.uniform(lo, hi) * 4) / 4 for lo, hi in ((0, 300), (0, 200), (10, 120), (10, 120)))
                coco['annotations'].append({'id': len(coco['annotations']) + 1, 'image_id': ids[i], 'category_id': 10 + c,
                                            'bbox': [float(x), float(y), float(w), float(h)], 'area': float(w * h), 'iscrowd': int(rs.rand() < 0.1)})
                for _ in range(rs.randint(0, 3)):
                    j = np.round(rs.uniform(-0.15, 0.15, 4) * np.array([w, h, w, h]) * 4) / 4
                    B.append(np.array([x + j[0], y + j[1], x + w + j[2], y + h + j[3]], dtype=np.float32))
                    Cl.append(c)
                    Sc.append(np.float32(rs.randint(1, levels) / levels))
            for _ in range(rs.randint(0, per_image)):
                x, y = rs.uniform(0, 300), rs.uniform(0, 200)
                B.append(np.round(np.array([x, y, x + rs.uniform(5, 100), y + rs.uniform(5, 100)]) * 4).astype(np.float32) / 4)
                Cl.append(c)
                Sc.append(np.float32(rs.randint(1, levels) / levels))
        preds.append([B, Cl, Sc])
    return coco, ids, preds, {c: 10 + c for c in range(n_cats)}


def stub_learner(d, images=None, targets=None):
    "an ImageLearner around the validation images and targets only: `predictions=` bypasses predict"
    from neuralnetworklibrary_amd.Applications import Vision as V
    learner = V.ImageLearner.__new__(V.ImageLearner)
    learner.target_type, learner.PATH = 'bbox', None
    val_ds = types.SimpleNamespace(images=[{'id': ID} for ID in d.ids] if images is None else images, y=d.targets if targets is None else targets)
    learner.data = types.SimpleNamespace(val_ds=val_ds, categories=d.categories, cat2dscat=d.cat2dscat, target_type='bbox')
    return learner


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_restatement_matches_golden():
    from neuralnetworklibrary_amd.Applications import Vision as V
    d = _Data.get()
    G, p = d.G, d.packed
    dtm, dtig, npig, gtig = d.r_match
    ann_id = np.concatenate([[0], np.array([a['id'] for a in d.coco['annotations']])[p['gt_ann']]])
    first_gt = np.repeat(p['gt_off'][:-1], np.diff(p['dt_off']))
    ids = np.where(dtm != 0, ann_id[np.where(dtm != 0, dtm + first_gt, 0)], 0)
    assert np.array_equal(ids, G['ev.dtm_id']) and np.array_equal(dtm != 0, G['ev.dtm_id'] != 0)
    assert np.array_equal(dtig, G['ev.dtig']) and np.array_equal(npig, G['ev.npig']) and np.array_equal(gtig, G['ev.gtig'])
    precision, recall, scores = d.r_acc
    assert np.array_equal(precision, G['precision']) and np.array_equal(recall, G['recall']) and np.array_equal(scores, G['scores'])
    stats, lines = V.coco_summarize(precision, recall, d.thr, S['maxDets'], ['all', 'small', 'medium', 'large'])
    assert np.array_equal(stats, G['stats']) and len(lines) == 12
    assert np.array_equal(np.isnan(d.r_map), np.isnan(G['mAP1']))
    assert np.allclose(d.r_map, G['mAP1'], rtol=0, atol=1e-12, equal_nan=True)
    # the degenerate corners the golden promises
    assert (G['precision'] == -1).mean() <= 0.5 and len(np.unique(G['precision'][G['precision'] > -1])) >= 30
    assert ((G['stats'] > -1) & (G['stats'] < 1)).all() and not np.array_equal(G['precision'][..., 1], G['precision'][..., 2])


def test_golden_inputs_are_what_the_tool_builds():
    d = _Data.get()
    for k, v in GEN.flat_inputs(d.coco, d.ids, d.preds).items():
        assert np.array_equal(v, d.G[k]), k


def test_pack_layout():
    from neuralnetworklibrary_amd import ops
    d = _Data.get()
    p, G = d.packed, d.G
    groups = np.stack([p['cat_ids'][p['grp_cat']], p['img_ids'][p['grp_img']], np.diff(p['dt_off']), np.diff(p['gt_off'])], axis=1)
    assert np.array_equal(groups, G['ev.groups'])                            # (sorted category, ascending image id), cut at 100
    assert np.array_equal(p['cat_ids'], np.sort(S['cat_ids'])) and np.array_equal(p['img_ids'], np.sort(d.ids))
    assert np.diff(p['dt_off']).max() == 100 and np.diff(p['gt_off']).max() >= 70
    for off, n in ((p['dt_off'], len(p['dt_score'])), (p['gt_off'], len(p['gt_area']))):
        assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all() and off.dtype == np.int32
    assert np.array_equal(p['cat_dt_off'], p['dt_off'][p['cat_grp_off']]) and p['cat_grp_off'][-1] == len(groups)
    for g in range(len(groups)):                                             # descending score inside a group, ranks from 0
        s = p['dt_score'][p['dt_off'][g]:p['dt_off'][g + 1]]
        assert (np.diff(s) <= 0).all()
        assert np.array_equal(p['dt_rank'][p['dt_off'][g]:p['dt_off'][g + 1]], np.arange(len(s)))
    for k in range(p['K']):                                                  # per category: stable descending score over (group, rank)
        a, z = p['cat_dt_off'][k], p['cat_dt_off'][k + 1]
        assert np.array_equal(p['order'][a:z], a + np.argsort(-p['dt_score'][a:z], kind='stable'))
    # the width is subtracted in the dtype the box arrives in (float32 from predict), then widened
    box32 = np.array([0.1, 0.2, 100.3, 50.7], dtype=np.float32)
    one = {'images': [{'id': 5}], 'categories': [{'id': 1}], 'annotations': [{'id': 1, 'image_id': 5, 'category_id': 1, 'bbox': [0, 0, 9, 9],
                                                                             'area': 81, 'iscrowd': 0}]}
    q = ops.det_eval_pack([[[box32], [0], [np.float32(0.5)]]], coco=one, image_ids=[5], cat2dscat={0: 1})
    assert q['dt_box'][0, 2] == float(box32[2] - box32[0]) != float(box32[2]) - float(box32[0])
    assert q['dt_box'][0, 3] == float(box32[3] - box32[1]) and q['dt_box'][0, 0] == float(box32[0])
    q = ops.det_eval_pack([[[[0.1, 0.2, 100.3, 50.7]], [0], [0.5]]], coco=one, image_ids=[5], cat2dscat={0: 1})
    assert q['dt_box'][0, 2] == 100.3 - 0.1
    # the mAP layout: groups by (category, image), float32 min-max boxes, counts per category
    m = d.mpacked
    assert m['pr_box'].dtype == np.float32 and m['gt_box'].dtype == np.float32 and len(m['pr_score']) == sum(len(x[0]) for x in d.preds)
    assert np.array_equal(m['ntrue'], np.bincount([c for y in d.targets for _, c in y], minlength=5))
    key = m['grp_cat'].astype(np.int64) * m['N'] + m['grp_img']
    assert (np.diff(key) > 0).all() and np.array_equal(m['cat_pr_off'], m['pr_off'][m['cat_grp_off']])


def test_value_errors():
    import copy
    from neuralnetworklibrary_amd import ops
    from neuralnetworklibrary_amd.Applications import Vision as V
    d = _Data.get()
    zero = copy.deepcopy(d.coco)
    zero['annotations'][3]['id'] = 0
    with pytest.raises(ValueError, match='id 0'):
        stub_learner(d).coco_pascal_eval(zero, predictions=d.preds)
    with pytest.raises(ValueError, match="no 'id'"):
        stub_learner(d, images=[{'id': ID} for ID in d.ids[:-1]] + [{'scale': 1.0}]).coco_pascal_eval(d.coco, predictions=d.preds)
    with pytest.raises(ValueError, match='absent from the category map'):
        stub_learner(d).coco_pascal_eval(d.coco, predictions=d.preds, cat2dscat={0: 7, 1: 3})
    with pytest.raises(ValueError, match='no prediction'):
        stub_learner(d).coco_pascal_eval(d.coco, predictions=[[[], [], []] for _ in d.ids])
    flat = [list(y) for y in d.targets]
    flat[0] = flat[0] + [(np.array([5., 5., 5., 9.]), 0)]
    with pytest.raises(ValueError, match='no positive area'):
        V.mAP_device(d.preds, flat, d.categories, verbose=False)
    with pytest.raises(ValueError, match=r'lie in \[0, 5\)'):
        ops.det_eval_pack([[[np.zeros(4, np.float32)], [5], [0.5]]] + d.preds[1:], targets=d.targets, n_categories=5)
    # a bad offset never reaches the device
    bad = dict(d.packed, dt_off=d.packed['dt_off'].copy())
    bad['dt_off'][3] = bad['dt_off'][4] + 1
    with pytest.raises(ValueError, match='non-decreasing'):
        ops.det_eval_coco(bad, S['iouThrs'], S['recThrs'], S['maxDets'], S['areaRng'])
    short = dict(d.mpacked, pr_off=d.mpacked['pr_off'][:-1])
    with pytest.raises(ValueError, match='offsets pr_off'):
        ops.det_map(short, S['mAP_thresholds'])
    with pytest.raises(ValueError, match='maxDets'):
        ops.det_eval_coco(d.packed, S['iouThrs'], S['recThrs'], [1, 10, 50], S['areaRng'])


def test_ops_refuse_cpu():
    from neuralnetworklibrary_amd import ops
    from neuralnetworklibrary_amd._lib import NnlError
    d = _Data.get()
    with pytest.raises(NnlError):
        ops.det_eval_coco(d.packed, S['iouThrs'], S['recThrs'], S['maxDets'], S['areaRng'], device='cpu')
    with pytest.raises(NnlError):
        ops.det_map(d.mpacked, S['mAP_thresholds'], device='cpu')


def test_c_entries_validate_before_any_hip_call():
    import ctypes
    from neuralnetworklibrary_amd._lib import lib
    one = ctypes.c_void_p(16)                                                # a non-null pointer that is never followed
    thr = (ctypes.c_double * 2)(0.5, 0.75)
    rng = (ctypes.c_double * 2)(0.0, 1e10)
    down = (ctypes.c_double * 2)(0.5, 0.25)
    md = (ctypes.c_int32 * 1)(100)
    hp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    match = lambda NG, T, A: lib.nnl_det_coco_match(one, one, one, one, one, one, one, NG, 4, 4, hp(thr), T, hp(rng), A, None, 0, one, one, one, one, None)
    assert match(0, 2, 1) == -1 and b'det_coco_match' in lib.nnl_last_error()
    assert match(1, 17, 1) == -1 and match(1, 2, 9) == -1 and match(1 << 31, 2, 1) == -1
    assert lib.nnl_det_coco_match(one, one, one, one, one, one, one, 1, 4, 4, hp(thr), 2, hp(rng), 1, None, 64, one, one, one, one, None) == -1
    acc = lambda rec, R, M: lib.nnl_det_coco_accumulate(one, one, one, one, one, one, one, one, 2, 3, 4, 2, 1, hp(md), M, hp(rec), R, one, one, one, None)
    assert acc(down, 2, 1) == -1 and b'ascend' in lib.nnl_last_error()
    assert acc(thr, 129, 1) == -1 and acc(thr, 2, 9) == -1 and acc(thr, 2, 0) == -1
    assert lib.nnl_det_map_match(one, one, one, one, 1, 4, 4, hp(thr), 0, one, None) == -1
    assert lib.nnl_det_map_match(one, one, None, one, 1, 4, 4, hp(thr), 2, one, None) == -1
    assert lib.nnl_det_map_integrate_workspace_bytes(10, 2) == 160 and lib.nnl_det_map_integrate_workspace_bytes(-1, 2) == 0
    assert lib.nnl_det_map_integrate(one, one, one, one, one, 3, 10, 2, one, 159, one, None) == -4
    assert lib.nnl_det_map_integrate(one, one, one, one, one, 0, 10, 2, one, 160, one, None) == -1


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_hip_coco_match_equals_golden():
    from neuralnetworklibrary_amd import ops
    d = _Data.get()
    off, doubles = ops._coco_scratch(d.packed, len(d.rng), len(d.thr))
    assert (off >= 0).any() and (off < 0).any() and doubles > ops.DET_EVAL_LDS_DOUBLES      # both homes of the overlap matrix are used
    dtm, dtig, npig = ops.det_eval_coco_match(d.packed, d.thr, d.rng)
    assert np.array_equal(dtm != 0, d.G['ev.dtm_id'] != 0) and np.array_equal(dtig, d.G['ev.dtig']) and np.array_equal(npig, d.G['ev.npig'])
    assert np.array_equal(dtm, d.r_match[0])                                 # the matched ground truth itself, not only "matched"


@pytest.mark.gpu
def test_hip_coco_eval_equals_golden_and_repeats():
    from neuralnetworklibrary_amd import ops
    d = _Data.get()
    first = ops.det_eval_coco(d.packed, S['iouThrs'], S['recThrs'], S['maxDets'], S['areaRng'])
    for got, name in zip(first, ('precision', 'recall', 'scores')):
        bad = np.nonzero(got != d.G[name])
        assert np.array_equal(got, d.G[name]), '%s differs at %d entries, first %r: %r vs %r' % (
            name, len(bad[0]), tuple(int(b[0]) for b in bad), got[bad][:1], d.G[name][bad][:1])
    again = ops.det_eval_coco(d.packed, S['iouThrs'], S['recThrs'], S['maxDets'], S['areaRng'])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


@pytest.mark.gpu
def test_hip_coco_pascal_eval_returns_the_stats(capsys, tmp_path):
    import json
    from neuralnetworklibrary_amd.General.Learner import Learner
    d = _Data.get()
    learner = stub_learner(d)
    learner.PATH = str(tmp_path) + os.sep
    assert Learner.verbose
    stats = learner.coco_pascal_eval(d.coco, predictions=d.preds)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith(' Average')]
    assert np.array_equal(stats, d.G['stats']) and stats.shape == (12,)
    assert len(lines) == 12 and lines[0].endswith('= %0.3f' % d.G['stats'][0]) and 'maxDets=  1' in lines[6]
    assert np.array_equal(learner.coco_eval['precision'], d.G['precision']) and np.array_equal(learner.coco_eval['recall'], d.G['recall'])
    assert not os.path.exists(os.path.join(str(tmp_path), 'preds.json'))     # written only on request
    del learner.data.cat2dscat                                               # the map falls back to the json's category order
    assert np.array_equal(learner.coco_pascal_eval(d.coco, predictions=d.preds, save_preds=True), d.G['stats'])
    rows = json.load(open(os.path.join(str(tmp_path), 'preds.json')))
    box = d.preds[0][0][0]
    assert len(rows) == sum(len(p[0]) for p in d.preds) and rows[0] == {
        'image_id': d.ids[0], 'category_id': d.cat2dscat[d.preds[0][1][0]], 'score': float(d.preds[0][2][0]),
        'bbox': [float(box[0]), float(box[1]), float(box[2] - box[0]), float(box[3] - box[1])]}


@pytest.mark.gpu
def test_hip_map_flags_and_values():
    from neuralnetworklibrary_amd import ops
    d = _Data.get()
    thr = S['mAP_thresholds']
    flags = ops.det_map_match(d.mpacked, thr)
    assert np.array_equal(flags, d.r_flags)
    vals = ops.det_map(d.mpacked, thr)
    host, L = host_map1(d.preds, d.targets, len(d.categories), thr)
    assert vals.shape == host.shape == (len(thr), 5)
    assert np.array_equal(np.isnan(vals), np.isnan(host)) and np.isnan(vals[:, S['no_gt']]).all()        # nan where the host gives nan
    assert np.array_equal(vals == 0, host == 0) and (vals[:, S['no_dt']] == 0).all()                     # 0.0 where the host gives 0.0
    ok = np.isfinite(host)
    err = np.abs(vals - host)[ok]
    bound = (np.broadcast_to(L, host.shape) * EPS * np.abs(host))[ok]
    print('mAP1 device vs host: max error', err.max(), 'bound at it', bound[err.argmax()])
    assert (err <= bound).all()
    assert np.allclose(vals, d.G['mAP1'], rtol=0, atol=1e-9, equal_nan=True)
    assert ops.det_map(d.mpacked, thr).tobytes() == vals.tobytes()           # no floating-point atomics


@pytest.mark.gpu
def test_hip_compute_map_device_agrees_with_host():
    d = _Data.get()
    learner = stub_learner(d)
    thr = S['mAP_thresholds']
    with np.errstate(all='ignore'):
        assert np.isnan(learner.compute_mAP(predictions=d.preds)) and np.isnan(learner.compute_mAP(predictions=d.preds, device=True))
    # the working categories alone, renumbered: a finite mean
    back = {c: i for i, c in enumerate(S['working'])}
    preds = [[[b for b, c in zip(B, Cl) if c in back], [back[c] for c in Cl if c in back], [s for s, c in zip(Sc, Cl) if c in back]]
             for B, Cl, Sc in d.preds]
    targets = [[(b, back[c]) for b, c in y if c in back] for y in d.targets]
    learner = stub_learner(d, targets=targets)
    learner.data.categories = {i: 'w%d' % i for i in range(3)}
    host = learner.compute_mAP(predictions=preds, mAP_thresholds=thr)
    dev = learner.compute_mAP(predictions=preds, mAP_thresholds=thr, device=True)
    L = max(sum(1 for p in preds for c in p[1] if c == k) for k in range(3))
    print('compute_mAP host', host, 'device', dev)
    assert 0 < host < 1 and abs(dev - host) <= (L + 3 * len(thr)) * EPS * host        # each value within L eps, the mean of T C values


@pytest.mark.gpu
def test_hip_tile_edges_against_restatement():
    """More than one 256-element tile per curve, runs of equal scores across tile edges (8 score levels), groups of every small size."""
    from neuralnetworklibrary_amd import ops
    coco, ids, preds, cat2dscat = random_set(23, 60, 2, 30, 8)
    p = ops.det_eval_pack(preds, coco=coco, image_ids=ids, cat2dscat=cat2dscat, max_det=20)
    assert np.diff(p['cat_dt_off']).min() > 2 * 256 and np.diff(p['dt_off']).max() == 20
    thr, rng, rec, md = np.array([0.5, 0.75]), np.array([[0, 1e10], [0, 48.0 ** 2]]), np.linspace(0, 1, 11), [3, 20]
    want = r_coco_accumulate(p, *r_coco_match(p, thr, rng)[:3], rec, md)
    got = ops.det_eval_coco(p, thr, rec, md, rng)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    targets = GEN.targets_of(coco, ids, cat2dscat)
    m = ops.det_eval_pack(preds, targets=targets, n_categories=2)
    flags = ops.det_map_match(m, [0.5, 0.75])
    want_flags = r_map_match(m, [0.5, 0.75])
    assert np.array_equal(flags, want_flags) and flags.any()
    vals, want_vals = ops.det_map(m, [0.5, 0.75]), r_map_integrate(m, want_flags)
    L = np.diff(m['cat_pr_off'])
    assert L.min() > 2 * 256 and (np.abs(vals - want_vals) <= L * EPS * want_vals).all() and (vals > 0).all()


@pytest.mark.gpu
def test_hip_single_group():
    "one image, one ground truth, one detection"
    from neuralnetworklibrary_amd import ops
    coco = {'images': [{'id': 9}], 'categories': [{'id': 4}],
            'annotations': [{'id': 1, 'image_id': 9, 'category_id': 4, 'bbox': [10., 10., 50., 40.], 'area': 2000., 'iscrowd': 0}]}
    preds = [[[np.array([10., 10., 60., 45.], dtype=np.float32)], [0], [np.float32(0.75)]]]             # overlap 1750 / 2000 = 0.875
    p = ops.det_eval_pack(preds, coco=coco, image_ids=[9], cat2dscat={0: 4})
    thr, rng = np.asarray(S['iouThrs']), np.asarray(S['areaRng'], dtype=np.float64)
    precision, recall, scores = ops.det_eval_coco(p, thr, S['recThrs'], S['maxDets'], rng)
    want = r_coco_accumulate(p, *r_coco_match(p, thr, rng)[:3], S['recThrs'], S['maxDets'])
    assert all(np.array_equal(g, w) for g, w in zip((precision, recall, scores), want))
    hit = thr <= 0.875
    assert (precision[hit][:, :, 0, 0, :] == 1 / (1 + np.spacing(1))).all() and (precision[~hit][:, :, 0, 0, :] == 0).all() and hit.sum() == 8
    assert (recall[hit][:, 0, 0, :] == 1).all() and (scores[hit][:, :, 0, 0, :] == 0.75).all()
    assert (precision[:, :, 0, 1, :] == -1).all() and (precision[:, :, 0, 3, :] == -1).all()          # no small, no large ground truth
    m = ops.det_eval_pack(preds, targets=[[(np.array([10., 10., 60., 50.]), 0)]], n_categories=1)
    vals = ops.det_map(m, [0.5, 0.875, 0.9])
    assert vals.tolist() == [[1.0], [0.0], [0.0]]                            # strictly above the threshold
