"""The multi-label image workflow (the Planet notebook) on the GPU: ResNet-34 + default head, 17 categories, bs 64, fed by
device_data.ImageBatches at 64^2, 128^2 and 256^2 (ImageLearner.data_resize between the sizes).
(1) Learner.train1minibatch, eager and replayed (use_graphs), with the default HIP loss (HipBCEWithLogitsLoss) against
    nn.BCEWithLogitsLoss() passed as loss_func — what the step ran before the kernels existed; the two alternate in one process
    and the spread of the rounds is printed next to the medians;
(2) one validation pass with the five F2 metrics on the kernel path (HIP loss + ops.fbeta) against the torch path (torch loss + the
    torch expression of fbeta_loss);
(3) ImageLearner.TTA('val') wall time against five separate loaders that each upload the set.
Usage: python tools/bench_multilabel.py [--sizes 64 128 256] [--bs 64] [--steps 20] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import device_data  # noqa: E402
from neuralnetworklibrary_amd.Applications import Vision as V  # noqa: E402
from neuralnetworklibrary_amd.General.Learner import HipBCEWithLogitsLoss, Learner  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128, 256])
ap.add_argument('--bs', type=int, default=64)
ap.add_argument('--train-images', type=int, default=256)
ap.add_argument('--val-images', type=int, default=128)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--rounds', type=int, default=3)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
NCAT = 17
THRESHOLDS = [0.1, 0.2, 0.3, 0.4, 0.5]
Learner.verbose = False
PATH = '/tmp/nnl_bench_multilabel'


class TorchF2(object):
    "fbeta_loss(2, threshold) as the plain torch expression (General/LossesMetrics.py), whatever the device"
    def __init__(self, threshold):
        self.threshold = threshold

    def __call__(self, y_pred, y_true):
        y_pred = (y_pred.sigmoid() >= self.threshold).float()
        tp = (y_pred * y_true).sum(dim=1)
        p = tp / (y_pred.sum(dim=1) + 1e-9)
        r = tp / (y_true.sum(dim=1) + 1e-9)
        return torch.mean(5 * (p * r) / (4 * p + r + 1e-9))


rs = np.random.RandomState(0)
mk = lambda n: [{'img': rs.randint(0, 256, (rs.randint(256, 300), rs.randint(256, 300), 3)).astype(np.uint8),
                 'target': (rs.random_sample(NCAT) < 0.3).astype(np.int64)} for _ in range(n)]
train, val = mk(a.train_images), mk(a.val_images)
data = V.ImageDataObj(PATH, 'multi_label', {i: str(i) for i in range(NCAT)}, a.bs, V.get_transforms('TopDown', sz=a.sizes[0]), train, val)
torch.manual_seed(0)
net = V.ImageClassificationNet(data, V.models.resnet34())
learners = {'hip': V.ImageLearner(PATH, data, net, optimizer='SGD_Mom'),
            'torch': V.ImageLearner(PATH, data, net, optimizer='SGD_Mom', loss_func=nn.BCEWithLogitsLoss())}
assert isinstance(learners['hip'].loss_func, HipBCEWithLogitsLoss) and type(learners['torch'].loss_func) is nn.BCEWithLogitsLoss
lr = [1e-5] * len(net.layer_groups)
result = {'bs': a.bs, 'ncat': NCAT, 'train_images': a.train_images, 'val_images': a.val_images, 'sizes': {}}


def timed_ms(fn, n=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def steps(learner, n):
    done = 0
    while done < n:
        for x, y in data.train_dl:
            if x.shape[0] != a.bs:
                continue
            learner.train1minibatch(x, y, lr)
            done += 1
            if done == n:
                break


def alternate(fns, rounds):
    "{name: [ms per round]} with the candidates taking turns in one process"
    runs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            runs[k].append(fn())
    return runs


def summary(runs, base, cand):
    b, c = float(np.median(runs[base])), float(np.median(runs[cand]))
    spread = max(max(v) - min(v) for v in runs.values())
    return {base + '_ms': [round(v, 3) for v in runs[base]], cand + '_ms': [round(v, 3) for v in runs[cand]],
            base + '_median_ms': round(b, 3), cand + '_median_ms': round(c, 3), 'diff_ms': round(c - b, 3), 'spread_ms': round(spread, 3),
            'no_slower_within_spread': bool(c - b <= spread)}


for sz in a.sizes:
    for L in learners.values():
        L.data_resize(sz)
    out = {}
    for mode, graphs in (('eager', False), ('replayed', True)):
        for L in learners.values():
            L.use_graphs(graphs)
            L.init_optimizer(wd=1e-4)
            net.train()
            steps(L, 6)                                                  # warm-up: plans, code objects, the capture
        runs = alternate({k: (lambda L=L: timed_ms(lambda: steps(L, a.steps), a.steps)) for k, L in learners.items()}, a.rounds)
        out[mode] = summary(runs, 'torch', 'hip')
        print('%3d^2 %-8s step: torch loss %.3f ms, HIP loss %.3f ms (diff %+.3f ms, spread of the rounds %.3f ms)' % (
            sz, mode, out[mode]['torch_median_ms'], out[mode]['hip_median_ms'], out[mode]['diff_ms'], out[mode]['spread_ms']), flush=True)
    for L in learners.values():
        L.use_graphs(False)
    evals = {'hip': lambda: timed_ms(lambda: learners['hip'].evaluate('val', metrics=[V.fbeta_loss(2, th) for th in THRESHOLDS])),
             'torch': lambda: timed_ms(lambda: learners['torch'].evaluate('val', metrics=[TorchF2(th) for th in THRESHOLDS]))}
    alternate(evals, 1)
    out['validation_pass'] = summary(alternate(evals, a.rounds), 'torch', 'hip')
    print('%3d^2 validation pass (%d images, five F2): torch path %.3f ms, kernel path %.3f ms' % (
        sz, a.val_images, out['validation_pass']['torch_median_ms'], out['validation_pass']['hip_median_ms']), flush=True)

    L = learners['hip']

    def five_uploads():
        tfms, weights = L.tta_transforms(0.4)
        preds = []
        for k, tfm in enumerate(tfms):
            ds = V.ImageDataset(PATH, val, tfm, 'multi_label', 'val')
            preds.append(L.predict(device_data.ImageBatches(ds, a.bs, shuffle=False, seed=k))[0])
        return V.combine_preds(preds, 'multi_label', weights)
    tta = {'views': lambda: timed_ms(lambda: L.TTA('val')), 'five_uploads': lambda: timed_ms(five_uploads)}
    alternate(tta, 1)
    out['tta_val'] = summary(alternate(tta, a.rounds), 'five_uploads', 'views')
    print('%3d^2 TTA(val): five loaders that upload the set %.2f ms, five views of the resident set %.2f ms' % (
        sz, out['tta_val']['five_uploads_median_ms'], out['tta_val']['views_median_ms']), flush=True)
    result['sizes'][str(sz)] = out

print(json.dumps(result))
