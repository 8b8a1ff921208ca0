"""The vision data side on the GPU: (1) device time of the HIP augmenter (ops.image_aug) for the eval and the training transform at
bs x sz^2 from ~256 x 300 uint8 sources, against the HBM bound of its output traffic (12 B written per output pixel, plus 24 B read
and written by the lighting pass) at the copy rate DESIGN.md quotes; (2) Learner.train1minibatch of ResNet-34 fed by
device_data.ImageBatches against the same step fed one fixed synthetic batch: the difference is the loader's cost.
Usage: python tools/bench_image_pipeline.py [--bs 64] [--sz 224] [--steps 40] [--skip-step]"""
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
ap.add_argument('--bs', type=int, default=64)
ap.add_argument('--sz', type=int, default=224)
ap.add_argument('--images', type=int, default=512)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--skip-step', action='store_true')
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
COPY_TBS = 6.29                                    # DESIGN.md's measured device copy rate, TB/s

rs = np.random.RandomState(0)
images = [{'img': rs.randint(0, 256, (rs.randint(240, 273), rs.randint(280, 321), 3)).astype(np.uint8), 'target': i % 2}
          for i in range(a.images)]
tfm_eval, tfm_aug = V.get_transforms('SideOn', a.sz)
result = {'bs': a.bs, 'sz': a.sz, 'images': a.images, 'arena_MB': sum(im['img'].size for im in images) / 1e6}


def events_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


# ---- (1) the kernels alone ------------------------------------------------------------------------------------------
for name, tfm in (('eval', tfm_eval), ('train', tfm_aug)):
    dl = device_data.ImageBatches(V.ImageDataset('', images, tfm, 'single_label', 'train'), a.bs, shuffle=True, seed=1)
    idx = np.random.RandomState(1).permutation(a.images)[:a.bs]
    table = dl._table(np.random.RandomState(2), 0, idx)
    params = torch.from_numpy(table.view(np.uint8).reshape(a.bs, -1)).cuda()
    lighting = bool(tfm.bal_range)
    call = lambda: ops.image_aug(dl.arena, dl.desc, params, tfm.sz, tfm.stats, lighting=lighting)
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    loop_us = min(events_us(call, 200) for _ in range(3))
    # the same launches replayed from a captured graph: no host launch path between them
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
    graph_us = min(events_us(g.replay, 20) for _ in range(3)) / K
    bound_bytes = a.bs * a.sz * a.sz * (36 if lighting else 12)
    bound_us = bound_bytes / (COPY_TBS * 1e6)
    best = min(loop_us, graph_us)
    result[name] = {'loop_us': round(loop_us, 2), 'graph_us': round(graph_us, 2), 'bound_MB': round(bound_bytes / 1e6, 1),
                    'bound_us': round(bound_us, 2), 'fraction_of_bound': round(bound_us / best, 3),
                    'Mpix_per_s': round(a.bs * a.sz * a.sz / best, 1)}
    print('%-5s transform %d x %d^2: %.1f us per call in a loop, %.1f us replayed; HBM bound %.1f MB / %.2f TB/s = %.1f us -> %.0f %% of the bound'
          % (name, a.bs, a.sz, loop_us, graph_us, bound_bytes / 1e6, COPY_TBS, bound_us, 100 * bound_us / best), flush=True)
    del g, keep

# host side of one minibatch: the draws and the parameter table
dl = device_data.ImageBatches(V.ImageDataset('', images, tfm_aug, 'single_label', 'train'), a.bs, shuffle=True, seed=1)
t0 = time.perf_counter()
for b in range(20):
    dl._table(np.random.RandomState(b), 0, np.arange(a.bs))
result['host_table_ms'] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
print('host: draws + parameter table of one minibatch %.2f ms' % result['host_table_ms'], flush=True)

# ---- (2) the training step fed by the loader against a fixed batch ------------------------------------------------------
if not a.skip_step:
    Learner.verbose = False
    data = V.ImageDataObj('/tmp/nnl_bench_image_pipeline', 'single_label', {0: 'a', 1: 'b'}, a.bs, [tfm_eval, tfm_aug], images, images[:a.bs])
    torch.manual_seed(0)
    learner = Learner('/tmp/nnl_bench_image_pipeline', data, V.ImageClassificationNet(data, V.models.resnet34()), optimizer='SGD_Mom')
    learner.init_optimizer(wd=1e-4)
    learner.model.train()
    lr = [1e-3] * len(learner.model.layer_groups)
    lr = lr if len(lr) > 1 else lr[0]
    fixed = next(iter(data.train_dl))
    fixed = (fixed[0].clone(), fixed[1].clone())

    def fed_by_loader(n):
        done = 0
        while done < n:
            for x, y in data.train_dl:
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

    fed_fixed(8), fed_by_loader(8)                     # warm-up: plans, code objects, both feeds
    runs = {'fixed': [], 'loader': []}
    for _ in range(3):                                 # alternate the two feeds in one process
        runs['fixed'].append(ms_per_step(fed_fixed, a.steps))
        runs['loader'].append(ms_per_step(fed_by_loader, a.steps))
    fx, ld = float(np.median(runs['fixed'])), float(np.median(runs['loader']))
    result['step'] = {'fixed_ms': [round(v, 3) for v in runs['fixed']], 'loader_ms': [round(v, 3) for v in runs['loader']],
                      'fixed_median_ms': round(fx, 3), 'loader_median_ms': round(ld, 3), 'loader_cost_ms': round(ld - fx, 3),
                      'img_per_s_fixed': round(a.bs / fx * 1e3, 1), 'img_per_s_loader': round(a.bs / ld * 1e3, 1)}
    print('ResNet-34 train1minibatch bs %d: fixed batch %.2f ms, fed by ImageBatches %.2f ms -> loader cost %.2f ms per step (%.1f %%)'
          % (a.bs, fx, ld, ld - fx, 100 * (ld - fx) / fx), flush=True)

print(json.dumps(result))
