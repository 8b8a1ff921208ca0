"""Detection evaluation at COCO-val size: `--images` images (5000), 80 categories, about 7 ground truths and up to 100 detections per
image (synthetic: a jittered detection for most ground truths, the rest false positives with categories of their own).  Both
protocols: the COCO / Pascal protocol (ops.det_eval_pack -> ops.det_eval_coco -> Vision.coco_summarize) and the mean average
precision (ops.det_eval_pack -> ops.det_map).

Reported per protocol (medians over `--rounds` alternations with the host baselines, after one warm-up of everything; spread = max -
min):
  pack_ms      ops.det_eval_pack: pure numpy on the host, no device
  ops_ms       the ONE upload and the launches, host clock around a device synchronise
  kernels_ms   the launches alone, from the library's HIP events (nnl_prof), next to the traffic bound: every input read once, the
               matcher's flags written once and read once, every output written once, over the 6.29 TB/s copy rate
  back_ms      the ONE copy back and the summary (twelve numbers / the mean)
  total_ms     pack + ops + back
Baselines, on the host:
  `host_mAP`   Vision.mAP, the triple Python loop (category, threshold, image)
  `numpy_coco` a numpy restatement of COCOeval.evaluate / accumulate written here (`numpy_coco`): per group the overlap matrix in
               numpy, the greedy matching in Python per (area range, threshold), per (category, area, maxDets) the cumulative sums over
               all thresholds at once.  Checked against the device result on the timed images before anything is timed.
Either baseline is timed on the first `--host-images` images; if that predicts more than a minute for all images the figure for all
images is that time scaled by the image count and labelled EXTRAPOLATED, else all images are timed.
Run it under a time limit of its own, e.g. `timeout 900 python tools/bench_det_eval.py`.
Usage: python tools/bench_det_eval.py [--images 5000] [--rounds 3] [--host-images 500]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import _lib, ops  # noqa: E402
from neuralnetworklibrary_amd.Applications import Vision as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--images', type=int, default=5000)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--host-images', type=int, default=500)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
HBM = 6.29e12
K = 80
IOU, REC, MAXDETS = np.linspace(.5, .95, 10), np.linspace(0, 1, 101), [1, 10, 100]
AREA = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
LBL = ['all', 'small', 'medium', 'large']


def synth(n_images, seed=0):
    rs = np.random.RandomState(seed)
    ids = (rs.permutation(n_images) + 1).tolist()
    coco = {'images': [{'id': i} for i in ids], 'categories': [{'id': k + 1} for k in range(K)], 'annotations': []}
    popular = np.cumsum(1.0 / np.arange(1, K + 1))
    preds = []
    for i in range(n_images):
        g = rs.poisson(7)
        cats = np.searchsorted(popular, rs.uniform(0, popular[-1], g))
        wh = np.round(np.exp(rs.uniform(np.log(8), np.log(300), (g, 2))) * 4) / 4
        xy = np.round(rs.uniform(0, 340, (g, 2)) * 4) / 4
        for j in range(g):
            coco['annotations'].append({'id': len(coco['annotations']) + 1, 'image_id': ids[i], 'category_id': int(cats[j]) + 1,
                                        'bbox': [float(xy[j, 0]), float(xy[j, 1]), float(wh[j, 0]), float(wh[j, 1])],
                                        'area': float(wh[j, 0] * wh[j, 1] * rs.uniform(0.5, 1.0)), 'iscrowd': int(rs.rand() < 0.05)})
        hit = rs.rand(g) < 0.7
        jit = np.round(rs.uniform(-0.12, 0.12, (g, 4)) * np.concatenate([wh, wh], axis=1) * 4) / 4
        near = (np.concatenate([xy, xy + wh], axis=1) + jit)[hit]
        n_fp = rs.randint(60, 101) - len(near)
        fxy, fwh = rs.uniform(0, 400, (n_fp, 2)), np.exp(rs.uniform(np.log(6), np.log(250), (n_fp, 2)))
        boxes = np.concatenate([near, np.round(np.concatenate([fxy, fxy + fwh], axis=1) * 4) / 4]).astype(np.float32)
        classes = np.concatenate([cats[hit], np.searchsorted(popular, rs.uniform(0, popular[-1], n_fp))]).astype(np.int64)
        scores = np.concatenate([rs.beta(4, 2, len(near)), rs.beta(1.2, 5, n_fp)]).astype(np.float32)
        preds.append([boxes, classes, scores])
    return coco, ids, preds


def targets_of(coco, ids):
    at = {ID: i for i, ID in enumerate(ids)}
    y = [[] for _ in ids]
    for ann in coco['annotations']:
        if not ann['iscrowd']:
            x, yy, w, h = ann['bbox']
            y[at[ann['image_id']]].append((np.array([x, yy, x + w, yy + h]), ann['category_id'] - 1))
    return y


def subset(coco, ids, preds, n):
    keep = set(ids[:n])
    return dict(coco, images=coco['images'][:n], annotations=[x for x in coco['annotations'] if x['image_id'] in keep]), ids[:n], preds[:n]


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def kernels_ms(fn):
    _lib.prof_enable(True)
    _lib.prof_collect()
    fn()
    torch.cuda.synchronize()
    ms = _lib.prof_collect()['elementwise']['ms']
    _lib.prof_enable(False)
    return ms


# ---- baseline: numpy restatement of COCOeval.evaluate / accumulate for boxes ---------------------------------------------------------

def numpy_coco(p):
    "precision [T, R, K, A, M], recall [T, K, A, M] from det_eval_pack's arrays (cocoeval.py:171-198, 243-428)"
    T, A, M, R, NG, Nd = len(IOU), len(AREA), len(MAXDETS), len(REC), len(p['grp_cat']), len(p['dt_score'])
    dtm, dtig, npig = np.zeros((A, T, Nd), bool), np.zeros((A, T, Nd), bool), np.zeros((A, NG), np.int64)
    d_area = p['dt_box'][:, 2] * p['dt_box'][:, 3]
    for g in range(NG):
        d0, d1, q0, q1 = p['dt_off'][g], p['dt_off'][g + 1], p['gt_off'][g], p['gt_off'][g + 1]
        D, G = p['dt_box'][d0:d1], p['gt_box'][q0:q1]
        crowd, area = (p['gt_flags'][q0:q1] & 1).astype(bool), p['gt_area'][q0:q1]
        w = np.minimum(D[:, None, 0] + D[:, None, 2], G[None, :, 0] + G[None, :, 2]) - np.maximum(D[:, None, 0], G[None, :, 0])
        h = np.minimum(D[:, None, 1] + D[:, None, 3], G[None, :, 1] + G[None, :, 3]) - np.maximum(D[:, None, 1], G[None, :, 1])
        inter, da = w * h, (D[:, 2] * D[:, 3])[:, None]
        with np.errstate(all='ignore'):
            iou = np.where((w <= 0) | (h <= 0), 0.0, inter / np.where(crowd[None, :], da, da + (G[:, 2] * G[:, 3])[None, :] - inter))
        for ai, (lo, hi) in enumerate(AREA):
            ig = (p['gt_flags'][q0:q1] & 2).astype(bool) | (area < lo) | (area > hi)
            npig[ai, g] = (~ig).sum()
            out_of_range = (d_area[d0:d1] < lo) | (d_area[d0:d1] > hi)
            if q0 == q1 or d0 == d1:
                dtig[ai, :, d0:d1] = out_of_range
                continue
            visit = np.argsort(ig, kind='stable')
            for t, thr in enumerate(IOU):
                taken = np.zeros(q1 - q0, bool)
                for d in range(d1 - d0):
                    bar, m = min(thr, 1 - 1e-10), -1
                    for j in visit:
                        if taken[j] and not crowd[j]:
                            continue
                        if m > -1 and not ig[m] and ig[j]:
                            break
                        if iou[d, j] < bar:
                            continue
                        bar, m = iou[d, j], j
                    if m >= 0:
                        taken[m], dtm[ai, t, d0 + d], dtig[ai, t, d0 + d] = True, True, ig[m]
                    else:
                        dtig[ai, t, d0 + d] = out_of_range[d]
    precision, recall = -np.ones((T, R, p['K'], A, M)), -np.ones((T, p['K'], A, M))
    for k in range(p['K']):
        g0, g1 = p['cat_grp_off'][k], p['cat_grp_off'][k + 1]
        order = p['order'][p['cat_dt_off'][k]:p['cat_dt_off'][k + 1]]
        for ai in range(A):
            n = npig[ai, g0:g1].sum()
            if g0 == g1 or n == 0:
                continue
            for m, md in enumerate(MAXDETS):
                kept = order[p['dt_rank'][order] < md]
                tp = np.cumsum(dtm[ai][:, kept] & ~dtig[ai][:, kept], axis=1).astype(np.float64)
                fp = np.cumsum(~dtm[ai][:, kept] & ~dtig[ai][:, kept], axis=1).astype(np.float64)
                for t in range(T):
                    rc, pr = tp[t] / n, tp[t] / (fp[t] + tp[t] + np.spacing(1))
                    recall[t, k, ai, m] = rc[-1] if len(kept) else 0
                    right = np.maximum.accumulate(pr[::-1])[::-1]
                    at = np.searchsorted(rc, REC, side='left')
                    q = np.zeros(R)
                    q[at < len(kept)] = right[at[at < len(kept)]]
                    precision[t, :, k, ai, m] = q
    return precision, recall


def host_or_extrapolated(name, fn_of_n, n_all, n_sub, rounds):
    "time fn_of_n(n_sub); all images only if that predicts under a minute"
    sub = [clock(lambda: fn_of_n(n_sub))[0] for _ in range(rounds)]
    scaled = float(np.median(sub)) * n_all / n_sub
    out = {'%s_on_%d_images_ms' % (name, n_sub): stat(sub)}
    if n_sub < n_all and scaled > 60e3:
        out['%s_EXTRAPOLATED_to_%d_images_ms' % (name, n_all)] = scaled
    elif n_sub < n_all:
        out['%s_all_images_ms' % name] = stat([clock(lambda: fn_of_n(n_all))[0] for _ in range(rounds)])
    return out


stat = lambda v: {'median': float(np.median(v)), 'spread': float(max(v) - min(v))}  # noqa: E731
coco, ids, preds = synth(a.images)
targets = targets_of(coco, ids)
categories = {k: 'c%d' % k for k in range(K)}
cat2dscat = {k: k + 1 for k in range(K)}
n_sub = min(a.host_images, a.images)
report = {'images': a.images, 'categories': K, 'ground_truths': len(coco['annotations']), 'detections': int(sum(len(p[0]) for p in preds)),
          'rounds': a.rounds}

# correctness on the timed subset, which also warms everything up
sc, si, sp = subset(coco, ids, preds, n_sub)
packed_sub = ops.det_eval_pack(sp, coco=sc, image_ids=si, cat2dscat=cat2dscat)
pr_dev, rc_dev, _ = ops.det_eval_coco(packed_sub, IOU, REC, MAXDETS, AREA)
pr_np, rc_np = numpy_coco(packed_sub)
assert np.array_equal(pr_dev, pr_np) and np.array_equal(rc_dev, rc_np), 'device and numpy COCO protocol differ'
with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
    host = V.mAP(sp, targets[:n_sub], categories, verbose=False)
    dev = V.mAP_device(sp, targets[:n_sub], categories, verbose=False)
assert (np.isnan(host) and np.isnan(dev)) or abs(host - dev) <= 1e-12 * abs(host), (host, dev)
ops.det_eval_coco(ops.det_eval_pack(preds, coco=coco, image_ids=ids, cat2dscat=cat2dscat), IOU, REC, MAXDETS, AREA)
ops.det_map(ops.det_eval_pack(preds, targets=targets, n_categories=K), V.COCO_thresholds)

T = {k: [] for k in ('coco_pack', 'coco_ops', 'coco_kernels', 'coco_back', 'map_pack', 'map_ops', 'map_kernels', 'map_back')}
for _ in range(a.rounds):
    t, packed = clock(lambda: ops.det_eval_pack(preds, coco=coco, image_ids=ids, cat2dscat=cat2dscat))
    T['coco_pack'].append(t)
    t, res = clock(lambda: ops._coco_launch(packed, IOU, AREA, 'cuda', REC, MAXDETS))
    T['coco_ops'].append(t)

    def coco_back():
        h = res['out'].cpu().numpy()
        n_pr, n_rc = int(np.prod(res['shape_pr'])), int(np.prod(res['shape_rc']))
        return V.coco_summarize(h[:n_pr].reshape(res['shape_pr']), h[2 * n_pr:2 * n_pr + n_rc].reshape(res['shape_rc']), IOU, MAXDETS, LBL)
    T['coco_back'].append(clock(coco_back)[0])
    T['coco_kernels'].append(kernels_ms(lambda: ops._coco_launch(packed, IOU, AREA, 'cuda', REC, MAXDETS)))
    t, mpacked = clock(lambda: ops.det_eval_pack(preds, targets=targets, n_categories=K))
    T['map_pack'].append(t)
    t, mres = clock(lambda: ops._map_launch(mpacked, V.COCO_thresholds, 'cuda', True))
    T['map_ops'].append(t)
    T['map_back'].append(clock(lambda: np.mean(mres['out'].cpu().numpy()))[0])
    T['map_kernels'].append(kernels_ms(lambda: ops._map_launch(mpacked, V.COCO_thresholds, 'cuda', True)))

Nd, Ng, NG = len(packed['dt_score']), len(packed['gt_area']), len(packed['grp_cat'])
A_, T_, M_, R_ = len(AREA), len(IOU), len(MAXDETS), len(REC)
coco_bytes = 48 * Nd + 41 * Ng + 16 * NG + 2 * 5 * A_ * T_ * Nd + 2 * 4 * A_ * NG + 8 * (2 * T_ * R_ * K * A_ * M_ + T_ * K * A_ * M_)
Np, Nt = len(mpacked['pr_score']), len(mpacked['gt_box'])
map_bytes = 28 * Np + 16 * Nt + 8 * len(mpacked['grp_cat']) + 2 * T_ * Np + 2 * 8 * T_ * Np + 8 * T_ * K
report['coco'] = {'groups': NG, 'detections_after_cut': Nd, 'pack_ms': stat(T['coco_pack']), 'ops_ms': stat(T['coco_ops']),
                  'kernels_ms': stat(T['coco_kernels']), 'traffic_bound_ms': coco_bytes / HBM * 1e3, 'back_ms': stat(T['coco_back']),
                  'total_ms': stat([x + y + z for x, y, z in zip(T['coco_pack'], T['coco_ops'], T['coco_back'])])}
report['map'] = {'groups': len(mpacked['grp_cat']), 'pack_ms': stat(T['map_pack']), 'ops_ms': stat(T['map_ops']),
                 'kernels_ms': stat(T['map_kernels']), 'traffic_bound_ms': map_bytes / HBM * 1e3, 'back_ms': stat(T['map_back']),
                 'total_ms': stat([x + y + z for x, y, z in zip(T['map_pack'], T['map_ops'], T['map_back'])])}
print('device', json.dumps({k: report[k] for k in ('coco', 'map')}), flush=True)


def host_map(n):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return V.mAP(preds[:n], targets[:n], categories, verbose=False)


def host_coco(n):
    c, i, p = subset(coco, ids, preds, n)
    return numpy_coco(ops.det_eval_pack(p, coco=c, image_ids=i, cat2dscat=cat2dscat))


report['map'].update(host_or_extrapolated('host_mAP', host_map, a.images, n_sub, a.rounds))
print('host_mAP done', flush=True)
report['coco'].update(host_or_extrapolated('numpy_coco', host_coco, a.images, n_sub, 1))
print(json.dumps(report))
