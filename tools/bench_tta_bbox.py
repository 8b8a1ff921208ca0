"""Detection test-time augmentation on the GPU: ImageLearner.TTA_bbox('val', transforms) at its defaults (device path: no device->host
copy inside the 5 L forwards, one merge kernel, one batched NMS) against the same computation written the reference's way: five
predict-style passes over the same five views with BBoxPredictor's per-image host copy, the undo in numpy (Vision.py:2092-2096) and
retinanet.nms per image on the concatenation.  The baseline clips to the image window as TTA_bbox does (BBoxPredictor's `window`), so
that the two results can be compared box for box: it is "the same semantics with a host copy per image", not code of an earlier tree.  ObjectDetectionNet(20) over `--images` resident ~495^2 uint8 images at batch size 1; the classifier's output
convolution gets seeded noise (std `--noise`), since a fresh net scores every anchor at its prior 0.01 and nothing passes thresh 0.05.
Both results are compared box for box before anything is timed.  One warm-up of each, then `--rounds` alternations; medians and spread.
Usage: python tools/bench_tta_bbox.py [--images 32] [--rounds 3] [--noise 0.1]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd.Applications import Vision as V  # noqa: E402
from neuralnetworklibrary_amd.Applications.VisionModels import retinanet as RN  # noqa: E402
from neuralnetworklibrary_amd.General.Core import TEN, to_cuda  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--images', type=int, default=32)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--noise', type=float, default=0.1)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'

rs = np.random.RandomState(0)
images = []
for i in range(a.images):
    H, W = rs.randint(490, 501, 2)
    images.append({'img': rs.randint(0, 256, (H, W, 3)).astype(np.uint8), 'target': [(np.array([20., 30., W - 40., H - 50.]), i % 20)],
                   'scale': 1.0, 'aspect_ratio': W / H})
tfms = V.get_transforms_bbox('SideOn', jitter=8, scale_range=[0.9, 1.0])
tmp = tempfile.mkdtemp()
data = V.ImageDataObj(tmp, 'bbox', {i: 'c%d' % i for i in range(20)}, 4, tfms, images[:4], images, seed=3)
torch.manual_seed(0)
net = V.ObjectDetectionNet(20)
torch.nn.init.normal_(net.classifier.output.weight, std=a.noise)
V.Learner.verbose = False
learner = V.ImageLearner(tmp, data, net, optimizer='SGD_Mom', loss_func=V.SSD_loss(0.5, 0.25, 2.0))


def baseline(thresh=0.05, max_overlap=0.5, rel_thresh=None, top_k=1000, max_boxes=20, dup=None, inc=None):
    "TTA_bbox as the reference writes it, on the loaders, the clip window and the device NMS of this library: a host copy per (pass, image), L more nms calls"
    dl = data.val_dl
    L = dl.n
    views = [dl.with_transform(tfms[0] if k == 0 else tfms[1], bs=1, seed=dl.seed + k) for k in range(5)]
    learner.model.eval()
    PB, PC, PS = [], [], []
    with torch.no_grad():
        for k, view in enumerate(views):
            for j, (x, _) in enumerate(view):
                x = to_cuda(x)
                anchors, reg, clas = learner.predict1minibatch(x)
                d = view.last_draws[j]
                window = (d['col_jit'], d['row_jit'], d['col_jit'] + d['rw'], d['row_jit'] + d['rh'])     # TTA_bbox clips to the image
                pred = learner.model.BBoxPredictor(x, reg, clas, anchors, thresh, max_overlap, rel_thresh, top_k, max_boxes, dup, inc, window)
                boxes, classes, scores = pred[0][0], pred[1][0], pred[2][0]
                if len(boxes) > 0:
                    boxes = np.array(boxes)
                    boxes = np.array([boxes[:, 0] - d['col_jit'], boxes[:, 1] - d['row_jit'], boxes[:, 2] - d['col_jit'], boxes[:, 3] - d['row_jit']]).T
                    boxes = (1 / (d['rand_scale'] * dl.scales[j])) * boxes
                    if d['flip'] == 1:
                        cols = dl.shapes[j][1]
                        boxes = np.array([cols - boxes[:, 2], boxes[:, 1], cols - boxes[:, 0], boxes[:, 3]]).T
                    boxes = list(boxes)
                PB.append(boxes); PC.append(classes); PS.append(scores)
        out = []
        for l in range(L):
            boxes, classes, scores = list(PB[l]), list(PC[l]), list(PS[l])
            for j in (l + L, l + 2 * L, l + 3 * L, l + 4 * L):
                boxes += list(PB[j]); classes += list(PC[j]); scores += list(PS[j])
            if not boxes:
                out.append([[], [], []])
                continue
            out.append(list(RN.nms(TEN(np.array(boxes), GPU=True), TEN(np.array(classes), GPU=True), TEN(np.array(scores), GPU=True),
                                   max_overlap, rel_thresh, top_k, max_boxes, dup, inc)))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


ours = lambda: learner.TTA_bbox('val', tfms)
_, want = timed(baseline)
_, got = timed(ours)                                                   # both warmed: every padded shape has run once
assert len(got) == len(want) == a.images
for (gb, gc, gs), (wb, wc, ws) in zip(got, want):
    assert len(gb) == len(wb) and [int(v) for v in gc] == [int(v) for v in wc]
    assert np.array_equal(np.array(gb, np.float32), np.array(wb, np.float32)) and np.array_equal(np.array(gs, np.float32), np.array(ws, np.float32))
t_ours, t_base = [], []
for _ in range(a.rounds):
    t_base.append(timed(baseline)[0])
    t_ours.append(timed(ours)[0])
spread = lambda v: max(v) - min(v)
print(json.dumps({'images': a.images, 'rounds': a.rounds, 'boxes_per_image_mean': float(np.mean([len(b) for b, _, _ in got])),
                  'tta_bbox_ms': {'median': float(np.median(t_ours)), 'spread': spread(t_ours), 'all': t_ours},
                  'baseline_ms': {'median': float(np.median(t_base)), 'spread': spread(t_base), 'all': t_base},
                  'results_equal': True}))
