"""The detection data side on the GPU: (1) device time of the HIP collater (ops.detect_aug) for one minibatch of bs samples padded to
pad x pad from ~495^2 uint8 sources, eval and training transform, against the HBM bound of its output write (12 B per output pixel)
at the copy rate DESIGN.md quotes; (2) Learner.train1minibatch of ObjectDetectionNet(20) + SSD_loss fed by
device_data.DetectionBatches against the same step fed one fixed minibatch of the same padded size: the difference is the loader's
cost.  The sources and the scale range are chosen so that EVERY minibatch pads to pad x pad (one input signature for the step).
Usage: python tools/bench_detection_pipeline.py [--bs 16] [--pad 512] [--steps 20] [--skip-step]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import device_data, ops  # noqa: E402
from neuralnetworklibrary_amd.Applications import Vision as V  # noqa: E402
from neuralnetworklibrary_amd.General.Learner import Learner  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--bs', type=int, default=16)
ap.add_argument('--pad', type=int, default=512)
ap.add_argument('--images', type=int, default=64)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--skip-step', action='store_true')
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
assert a.pad % 32 == 0 and a.pad >= 128
COPY_TBS = 6.29                                    # DESIGN.md's measured device copy rate, TB/s
JITTER = 8

# sources of pad - 22 .. pad - 12 pixels a side: at scale 1, rand_scale in [0.985, 1] and jitter <= 8 the largest resized side plus
# the jitter lies in (pad - 32, pad], so every minibatch pads to pad x pad
rs = np.random.RandomState(0)
images = []
for i in range(a.images):
    H, W = rs.randint(a.pad - 22, a.pad - 11, 2)
    target = []
    for _ in range(rs.randint(1, 9)):
        x0, y0 = rs.uniform(0, W - 40), rs.uniform(0, H - 40)
        target.append((np.array([x0, y0, rs.uniform(x0 + 20, W), rs.uniform(y0 + 20, H)]), int(rs.randint(0, 20))))
    images.append({'img': rs.randint(0, 256, (H, W, 3)).astype(np.uint8), 'target': target, 'scale': 1.0, 'aspect_ratio': W / H})
tfm_eval = V.TransformBBox('Basic', None, None, jitter=0, scale_range=[1, 1])
tfm_aug = V.TransformBBox('SideOn', jitter=JITTER, scale_range=[0.985, 1.0])
result = {'bs': a.bs, 'pad': a.pad, 'images': a.images, 'arena_MB': sum(im['img'].size for im in images) / 1e6}


def events_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


# ---- (1) the kernel alone ----------------------------------------------------------------------------------------------
for name, tfm in (('eval', tfm_eval), ('train', tfm_aug)):
    dl = device_data.DetectionBatches(V.ImageDataset('', images, tfm, 'bbox', 'train'), a.bs, grouped=True, seed=1)
    table, v = dl._table(np.random.RandomState(2), 0, dl.groups[0])
    assert (v['Hp'], v['Wp']) == (a.pad, a.pad), v
    params = torch.from_numpy(table.view(np.uint8).reshape(len(table), -1)).cuda()
    call = lambda: ops.detect_aug(dl.arena, dl.desc, dl.image_mean, dl.box_arena, dl.cat_arena, params, v['Hp'], v['Wp'], v['N'],
                                  v['row_jit'], v['col_jit'], v['rand_scale'], tfm.stats)
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    loop_us = min(events_us(call, 2000) for _ in range(3))              # about 60 ms per window
    # the same launch replayed from a captured graph: no host launch path between the kernels
    K = 20
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        for _ in range(K):
            keep = call()
    g.replay()
    torch.cuda.synchronize()
    graph_us = min(events_us(g.replay, 200) for _ in range(3)) / K       # 4000 launches, about 0.1 s per window
    bound_bytes = len(table) * a.pad * a.pad * 12
    bound_us = bound_bytes / (COPY_TBS * 1e6)
    best = min(loop_us, graph_us)
    result[name] = {'loop_us': round(loop_us, 2), 'graph_us': round(graph_us, 2), 'bound_MB': round(bound_bytes / 1e6, 1),
                    'bound_us': round(bound_us, 2), 'fraction_of_bound': round(bound_us / best, 3),
                    'Mpix_per_s': round(len(table) * a.pad * a.pad / best, 1)}
    print('%-5s transform %d x %d^2: %.1f us per call in a loop, %.1f us replayed; output-write bound %.1f MB / %.2f TB/s = %.1f us -> %.0f %% of the bound'
          % (name, len(table), a.pad, loop_us, graph_us, bound_bytes / 1e6, COPY_TBS, bound_us, 100 * bound_us / best), flush=True)
    del g, keep

# host side of one minibatch: the draws and the parameter table
dl = device_data.DetectionBatches(V.ImageDataset('', images, tfm_aug, 'bbox', 'train'), a.bs, grouped=True, seed=1)
t0 = time.perf_counter()
for b in range(20):
    dl._table(np.random.RandomState(b), 0, dl.groups[0])
result['host_table_ms'] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
print('host: draws + parameter table of one minibatch %.2f ms' % result['host_table_ms'], flush=True)

# ---- (2) the training step fed by the loader against a fixed minibatch -----------------------------------------------------
if not a.skip_step:
    Learner.verbose = False
    path = '/tmp/nnl_bench_detection_pipeline'
    data = V.ImageDataObj(path, 'bbox', {i: str(i) for i in range(20)}, a.bs, [tfm_eval, tfm_aug], images, images[:4])
    torch.manual_seed(0)
    learner = V.ImageLearner(path, data, V.ObjectDetectionNet(20), optimizer='SGD_Mom', loss_func=V.SSD_loss(0.5, 0.25, 2.0))
    learner.init_optimizer(wd=1e-4)
    learner.model.train()
    lr = [1e-3] * len(learner.model.layer_groups)
    fixed = next(iter(data.train_dl))
    fixed = (fixed[0].clone(), [t.clone() for t in fixed[1]])
    assert tuple(fixed[0].shape[2:]) == (a.pad, a.pad)

    def fed_by_loader(n):
        done = 0
        while done < n:
            for x, y in data.train_dl:
                assert x.shape == fixed[0].shape or x.shape[0] != a.bs
                learner.train1minibatch(x, y, lr)
                done += 1
                if done == n:
                    break

    def fed_fixed(n):
        for _ in range(n):
            learner.train1minibatch(fixed[0], fixed[1], lr)

    def ms_per_step(fn, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3

    fed_fixed(6), fed_by_loader(6)                     # warm-up: plans, code objects, both feeds
    runs = {'fixed': [], 'loader': []}
    for _ in range(3):                                 # alternate the two feeds in one process
        runs['fixed'].append(ms_per_step(fed_fixed, a.steps))
        runs['loader'].append(ms_per_step(fed_by_loader, a.steps))
    fx, ld = float(np.median(runs['fixed'])), float(np.median(runs['loader']))
    result['step'] = {'fixed_ms': [round(v, 3) for v in runs['fixed']], 'loader_ms': [round(v, 3) for v in runs['loader']],
                      'fixed_median_ms': round(fx, 3), 'loader_median_ms': round(ld, 3), 'loader_cost_ms': round(ld - fx, 3),
                      'img_per_s_fixed': round(a.bs / fx * 1e3, 1), 'img_per_s_loader': round(a.bs / ld * 1e3, 1)}
    print('RetinaNet train1minibatch bs %d at %d^2: fixed minibatch %.2f ms, fed by DetectionBatches %.2f ms -> loader cost %.2f ms per step (%.1f %%)'
          % (a.bs, a.pad, fx, ld, ld - fx, 100 * (ld - fx) / fx), flush=True)

print(json.dumps(result))
