"""Golden vectors G23 for detection evaluation: the COCO / Pascal protocol (reference Applications/Vision.py:2142-2177,
coco_pascal_eval -> Applications/pycocotools/cocoeval.py) and the mean average precision (Applications/Vision.py:1696-1800, mAP1 / mAP).

A synthetic annotation dict (`build()`: 40 images whose ids do not ascend, 5 categories whose ids are not in order) and predictions in
the predict('val') format are written to two temporary json files and run through the REAL reference's COCO, loadRes,
COCOeval(..., 'bbox'), evaluate, accumulate and summarize, loaded through oracle/_ref_import.py under three shims: `np.float = float`,
`np.linspace` with its `num` cast to int (the reference passes floats, which numpy 2 refuses), and pycocotools' compiled
`_mask.iou` replaced by `box_iou` below.  THE OVERLAP IS THEREFORE THIS TOOL'S RESTATEMENT of pycocotools' box IoU (six fp64
operations per pair), not compiled reference code; everything else — grouping, sorting, matching, accumulation, the twelve
summary numbers — is the reference's own Python.  With the same boxes as predictions / targets (the targets are the annotations that
are neither crowd nor ignored, as min-max boxes [x, y, x + w, y + h]) the tool also stores the real reference's Vision.mAP1 per
(category, threshold) and Vision.mAP.

The set is asserted not to be degenerate (see `check_set`): image ids out of order, a category without ground truth, one without
detections, an image with only detections and one with only ground truths, a group of 140 detections (the cuts at 100 and 10), a group
of 75 ground truths (more than a wave), crowd and 'ignore' annotations, areas in all three ranges and exactly 32^2 and 96^2, scores
quantised to k / 16 (ties everywhere), a detection identical to its ground truth, one with overlap exactly 0.5.
Writes data only: tests/golden/g23_det_eval.npz.  tests/test_det_eval.py imports SETTINGS, build and targets_of.
Usage: python tools/gen_golden_det_eval.py   (needs the reference checkout the oracle shim points at)"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g23_det_eval.npz')
SETTINGS = {'seed': 2300, 'n_images': 40, 'cat_ids': [7, 3, 11, 5, 9],       # model category i <-> dataset id cat_ids[i] (json order)
            'working': [0, 1, 4], 'no_gt': 2, 'no_dt': 3,
            'iouThrs': np.linspace(.5, .95, 10), 'recThrs': np.linspace(0, 1, 101), 'maxDets': [1, 10, 100],
            'areaRng': [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
            'mAP_thresholds': [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]}


def box_iou(d, g, iscrowd):
    "pycocotools' box IoU (maskApi.c bbIou) restated: [len(d), len(g)] overlaps of [x, y, w, h] boxes, fp64, one operation at a time"
    out = np.zeros((len(d), len(g)))
    for i, D in enumerate(d):
        for j, G in enumerate(g):
            w = min(float(D[0]) + float(D[2]), float(G[0]) + float(G[2])) - max(float(D[0]), float(G[0]))
            h = min(float(D[1]) + float(D[3]), float(G[1]) + float(G[3])) - max(float(D[1]), float(G[1]))
            if w <= 0 or h <= 0:
                continue
            inter, da = w * h, float(D[2]) * float(D[3])
            out[i, j] = inter / (da if iscrowd[j] else da + float(G[2]) * float(G[3]) - inter)
    return out


def build():
    """(coco annotation dict, image_ids in dataset order, predictions in the predict('val') format, cat2dscat, categories)"""
    S = SETTINGS
    rs = np.random.RandomState(S['seed'])
    N = S['n_images']
    ids = [int(v) * 3 + 11 for v in rs.permutation(N)]
    coco = {'images': [{'id': ids[i], 'file_name': 'img_%03d.jpg' % i, 'height': 480, 'width': 640} for i in range(N)],
            'categories': [{'id': c, 'name': 'c%d' % c} for c in S['cat_ids']], 'annotations': []}
    preds = [[[], [], []] for _ in range(N)]
    q = lambda v: float(np.round(v * 4) / 4)                                # quarter pixels: exact in float32

    def gt(i, c, x, y, w, h, crowd=0, ignore=None, area=None):
        a = {'id': len(coco['annotations']) + 1, 'image_id': ids[i], 'category_id': S['cat_ids'][c], 'bbox': [x, y, w, h],
             'area': float(w * h if area is None else area), 'iscrowd': crowd}
        if ignore is not None:
            a['ignore'] = ignore
        coco['annotations'].append(a)

    def dt(i, c, x0, y0, x1, y1, s):
        preds[i][0].append(np.array([x0, y0, x1, y1], dtype=np.float32))
        preds[i][1].append(c)
        preds[i][2].append(np.float32(s / 16))

    def random_gt(i, c):
        kind = rs.randint(0, 8)
        if kind == 0:
            w = h = 32.0
        elif kind == 1:
            w = h = 96.0
        else:
            lo, hi = [(8, 30), (33, 90), (100, 200)][kind % 3]
            w, h = q(rs.uniform(lo, hi)), q(rs.uniform(lo, hi))
        x, y = q(rs.uniform(0, 400)), q(rs.uniform(0, 250))
        crowd = int(rs.rand() < 0.15)
        ignore = (1 if rs.rand() < 0.1 else None) if not crowd else (0 if rs.rand() < 0.2 else None)
        area = None if kind < 2 or rs.rand() < 0.3 else float(np.round(w * h * rs.uniform(0.6, 1.0), 2))
        gt(i, c, x, y, w, h, crowd, ignore, area)
        return x, y, w, h

    def jittered(i, c, x, y, w, h, spread=0.2):
        dx0, dy0, dx1, dy1 = (q(rs.uniform(-spread, spread) * s) for s in (w, h, w, h))
        dt(i, c, max(0.0, x + dx0), max(0.0, y + dy0), x + w + dx1, y + h + dy1, rs.randint(1, 16))

    def false_positive(i, c):
        x, y = q(rs.uniform(0, 500)), q(rs.uniform(0, 350))
        dt(i, c, x, y, x + q(rs.uniform(6, 150)), y + q(rs.uniform(6, 150)), rs.randint(1, 12))

    # image 0: overlap exactly 0.5 (COCO matches it at t = 0.5, mAP1's strict test does not) and a detection identical to its ground truth
    gt(0, 0, 0.0, 0.0, 10.0, 10.0)
    dt(0, 0, 0.0, 0.0, 10.0, 5.0, 15)
    gt(0, 0, 100.0, 100.0, 40.0, 40.0)
    dt(0, 0, 100.0, 100.0, 140.0, 140.0, 14)
    # image 1: detections only; image 2: ground truths only
    for c in (0, 1, S['no_gt']):
        for _ in range(3):
            false_positive(1, c)
    for c in (0, 1, S['no_dt']):
        for _ in range(3):
            random_gt(2, c)
    # image 3: one group of 140 detections around 6 ground truths
    boxes = [random_gt(3, 0) for _ in range(6)]
    for n in range(140):
        if n % 3 == 2:
            false_positive(3, 0)
        else:
            jittered(3, 0, *boxes[n % 6], spread=0.3)
    # image 4: one group of 75 ground truths (a 15 x 5 grid) and 30 detections
    for n in range(75):
        x, y, w, h = 8.0 + 40.0 * (n % 15), 10.0 + 60.0 * (n // 15), q(rs.uniform(12, 36)), q(rs.uniform(12, 50))
        gt(4, 1, x, y, w, h, int(n % 9 == 4), 1 if n % 11 == 5 else None, float(np.round(w * h * rs.uniform(0.6, 1.0), 2)))
        if n % 5 < 2:
            jittered(4, 1, x, y, w, h)
    # the rest: a few objects per working category, detections around most of them, false positives, ties by quantised scores
    for i in range(5, N):
        for c in S['working']:
            for _ in range(rs.randint(0, 5)):
                b = random_gt(i, c)
                for _ in range(rs.choice([0, 1, 1, 1, 2])):
                    jittered(i, c, *b)
            for _ in range(rs.randint(0, 4)):
                false_positive(i, c)
        if rs.rand() < 0.3:
            false_positive(i, S['no_gt'])
        if rs.rand() < 0.3:
            random_gt(i, S['no_dt'])
    cat2dscat = {i: c for i, c in enumerate(S['cat_ids'])}
    categories = {i: 'c%d' % c for i, c in enumerate(S['cat_ids'])}
    return coco, ids, preds, cat2dscat, categories


def targets_of(coco, image_ids, cat2dscat):
    "val_ds.y for the mAP path: per image [(min-max box, model category), ...] of the annotations that are neither crowd nor ignored"
    back = {v: k for k, v in cat2dscat.items()}
    at = {ID: i for i, ID in enumerate(image_ids)}
    y = [[] for _ in image_ids]
    for a in coco['annotations']:
        if a.get('iscrowd', 0) or a.get('ignore', 0):
            continue
        x, yy, w, h = a['bbox']
        y[at[a['image_id']]].append((np.array([x, yy, x + w, yy + h]), back[a['category_id']]))
    return y


def flat_inputs(coco, image_ids, preds):
    anns = coco['annotations']
    return {'in.image_ids': np.array(image_ids, dtype=np.int64), 'in.cat_ids': np.array(SETTINGS['cat_ids'], dtype=np.int64),
            'in.pred_count': np.array([len(p[0]) for p in preds], dtype=np.int64),
            'in.pred_boxes': np.array([b for p in preds for b in p[0]], dtype=np.float32).reshape(-1, 4),
            'in.pred_classes': np.array([c for p in preds for c in p[1]], dtype=np.int64),
            'in.pred_scores': np.array([s for p in preds for s in p[2]], dtype=np.float32),
            'in.ann_id': np.array([a['id'] for a in anns], dtype=np.int64), 'in.ann_image': np.array([a['image_id'] for a in anns], dtype=np.int64),
            'in.ann_cat': np.array([a['category_id'] for a in anns], dtype=np.int64),
            'in.ann_bbox': np.array([a['bbox'] for a in anns], dtype=np.float64), 'in.ann_area': np.array([a['area'] for a in anns], dtype=np.float64),
            'in.ann_iscrowd': np.array([a['iscrowd'] for a in anns], dtype=np.int64),
            'in.ann_ignore': np.array([a.get('ignore', -1) for a in anns], dtype=np.int64)}


def check_set(coco, ids, preds):
    S = SETTINGS
    anns = coco['annotations']
    assert any(a > b for a, b in zip(ids, ids[1:])) and len(set(ids)) == len(ids), 'image ids must not ascend in list order'
    gt_cats = {a['category_id'] for a in anns}
    dt_cats = {S['cat_ids'][c] for p in preds for c in p[1]}
    assert S['cat_ids'][S['no_gt']] in dt_cats - gt_cats and S['cat_ids'][S['no_dt']] in gt_cats - dt_cats
    gt_imgs = {a['image_id'] for a in anns}
    assert any(len(p[0]) and ids[i] not in gt_imgs for i, p in enumerate(preds)), 'an image with detections and no ground truth'
    assert any(not len(p[0]) and ids[i] in gt_imgs for i, p in enumerate(preds)), 'an image with ground truths and no detection'
    assert max(sum(1 for c in p[1] if c == k) for p in preds for k in range(5)) >= 130
    per = {}
    for a in anns:
        per[a['image_id'], a['category_id']] = per.get((a['image_id'], a['category_id']), 0) + 1
    assert max(per.values()) >= 70
    crowd = np.mean([a['iscrowd'] for a in anns])
    assert 0.08 < crowd < 0.25, crowd
    assert any(a.get('ignore') == 1 and not a['iscrowd'] for a in anns) and any(a.get('ignore') == 0 and a['iscrowd'] for a in anns)
    areas = np.array([a['area'] for a in anns])
    assert (areas < 32 ** 2).any() and ((areas > 32 ** 2) & (areas < 96 ** 2)).any() and (areas > 96 ** 2).any()
    assert (areas == 32 ** 2).any() and (areas == 96 ** 2).any()
    assert all(float(s) * 16 == int(float(s) * 16) for p in preds for s in p[2])
    a0, a1 = anns[0], anns[1]
    assert a0['bbox'] == [0.0, 0.0, 10.0, 10.0] and preds[0][0][0].tolist() == [0.0, 0.0, 10.0, 5.0]
    assert box_iou([[0., 0., 10., 5.]], [a0['bbox']], [0])[0, 0] == 0.5
    x, y, w, h = a1['bbox']
    assert preds[0][0][1].tolist() == [x, y, x + w, y + h]


def main():
    from oracle import _ref_import
    mods = _ref_import.load()
    V = mods['Applications.Vision']
    # the three shims
    np.float = float
    linspace = np.linspace
    np.linspace = lambda start, stop, num=50, *a, **k: linspace(start, stop, int(num), *a, **k)
    sys.modules['pycocotools._mask'].iou = box_iou
    sys.modules['Applications.pycocotools.mask'].iou = box_iou
    COCO, COCOeval = V.COCO, V.COCOeval
    S = SETTINGS

    coco, ids, preds, cat2dscat, categories = build()
    check_set(coco, ids, preds)
    out = flat_inputs(coco, ids, preds)
    res = []
    for i, (B, Cl, Sc) in enumerate(preds):                                 # Vision.py:2158-2167
        for box, cat, score in zip(B, Cl, Sc):
            res.append({'image_id': ids[i], 'category_id': cat2dscat[cat], 'score': float(score),
                        'bbox': [float(box[0]), float(box[1]), float(box[2] - box[0]), float(box[3] - box[1])]})
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()) as log:
        json.dump(coco, open(os.path.join(tmp, 'val.json'), 'w'))
        json.dump(res, open(os.path.join(tmp, 'preds.json'), 'w'), indent=4)
        coco_true = COCO(os.path.join(tmp, 'val.json'))
        coco_pred = coco_true.loadRes(os.path.join(tmp, 'preds.json'))
        E = COCOeval(coco_true, coco_pred, 'bbox')
        E.params.imgIds = ids
        E.evaluate()
        E.accumulate()
        E.summarize()
    lines = [l for l in log.getvalue().splitlines() if l.startswith(' Average')]
    assert len(lines) == 12
    print('\n'.join(lines))
    p = E.params
    assert np.array_equal(p.iouThrs, S['iouThrs']) and np.array_equal(p.recThrs, S['recThrs']) and list(p.maxDets) == S['maxDets']
    assert [list(map(float, a)) for a in p.areaRng] == [list(map(float, a)) for a in S['areaRng']]
    K, A, I = len(p.catIds), len(p.areaRng), len(p.imgIds)
    dtm, dtig, gtig, npig = [[] for _ in range(A)], [[] for _ in range(A)], [[] for _ in range(A)], [[] for _ in range(A)]
    groups = []
    for k in range(K):
        for i in range(I):
            for a in range(A):
                e = E.evalImgs[k * A * I + a * I + i]
                if e is None:
                    continue
                if a == 0:
                    groups.append((int(p.catIds[k]), int(p.imgIds[i]), len(e['dtIds']), len(e['gtIds'])))
                dtm[a].append(np.asarray(e['dtMatches']).astype(np.int64).reshape(len(p.iouThrs), -1))
                dtig[a].append(np.asarray(e['dtIgnore']).astype(np.uint8).reshape(len(p.iouThrs), -1))
                gtig[a].append(np.asarray(e['gtIgnore']).astype(np.uint8).reshape(-1))
                npig[a].append(int(np.count_nonzero(np.asarray(e['gtIgnore']) == 0)))
    out['ev.groups'] = np.array(groups, dtype=np.int64)                      # (category id, image id, detections, ground truths) per group
    out['ev.dtm_id'] = np.stack([np.concatenate(x, axis=1) for x in dtm])    # [A, T, Nd]: id of the matched annotation, 0 = unmatched
    out['ev.dtig'] = np.stack([np.concatenate(x, axis=1) for x in dtig])     # [A, T, Nd]
    out['ev.gtig'] = np.stack([np.concatenate(x) for x in gtig])             # [A, Ng], each group in evaluateImg's ignore-last order
    out['ev.npig'] = np.array(npig, dtype=np.int32)                          # [A, NG]
    out['precision'], out['recall'], out['scores'] = E.eval['precision'], E.eval['recall'], E.eval['scores']
    out['stats'] = np.asarray(E.stats, dtype=np.float64)
    pr = out['precision']
    assert pr.shape == (10, 101, 5, 4, 3) and (pr == -1).mean() <= 0.5, (pr == -1).mean()
    assert len(np.unique(pr[pr > -1])) >= 30
    assert ((out['stats'] > -1) & (out['stats'] < 1)).all(), out['stats']
    assert not np.array_equal(pr[..., 1], pr[..., 2]) and not np.array_equal(pr[..., 0], pr[..., 1])
    assert (out['ev.dtm_id'][0, 0] != 0).any() and out['ev.dtig'].any() and max(g[2] for g in groups) == 100

    # the mean average precision of the same boxes, by the real reference
    targets = targets_of(coco, ids, cat2dscat)
    N, C, thr = len(preds), len(categories), S['mAP_thresholds']
    targs = [[[] for _ in range(N)] for _ in range(C)]
    pp = [[[] for _ in range(N)] for _ in range(C)]
    ss = [[[] for _ in range(N)] for _ in range(C)]
    for i in range(N):                                                      # Vision.py:1777-1786
        for j in range(len(preds[i][0])):
            pp[preds[i][1][j]][i].append(preds[i][0][j])
            ss[preds[i][1][j]][i].append(preds[i][2][j])
        for b, c in targets[i]:
            targs[c][i].append(b)
    vals = np.zeros((len(thr), C))
    with np.errstate(all='ignore'), contextlib.redirect_stdout(io.StringIO()):
        for c in range(C):
            for j, t in enumerate(thr):
                vals[j, c] = V.mAP1(targs[c], pp[c], ss[c], t)
        out['mAP'] = np.float64(V.mAP(preds, targets, categories, thr))
    out['mAP1'] = vals
    assert np.isnan(vals[:, S['no_gt']]).all() and (vals[:, S['no_dt']] == 0).all() and np.isfinite(vals[:, S['working']]).all()
    assert vals[0, 0] > vals[-1, 0] > 0, vals[:, 0]
    print('mAP1 [T, C]:\n', np.round(vals, 4))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, '%.1f KB' % (os.path.getsize(OUT) / 1024), '| groups', len(groups), 'detections', out['ev.dtm_id'].shape[-1],
          'ground truths', out['ev.gtig'].shape[-1])


if __name__ == '__main__':
    main()
