"""Line convolution (csrc/lineconv.hip, K19) at every distinct (1, T) / (T, 1) geometry of InceptionV4 at 299 x 299, bs 32: 64 -> 64 at
73 x 73 (T = 7), the 192 / 224 / 256 / 320 family at 17 x 17 (T = 7), 384 -> 256, 384 -> 448, 448 -> 512, 512 -> 256 at 8 x 8 (T = 3), both
orientations of each.  Forward, dgrad and wgrad through the C ABI (no autograd / Python overhead between the launches).

Per kernel: time per launch by HIP events — after a warm-up of every contender, three alternations of (ours, baseline a, baseline b) in
one process, each a block of `--iters` launches; the median of the three blocks with min and max — and that time against the bound
max(2 N H W T C K / 157.3 TFLOP/s, bytes touched once / 6.29 TB/s) computed from the shapes here, with the side that binds named.
The baselines live in this tool only and are never used by the package:
  (a) ATen's torch.nn.functional.conv2d with the padding tuple, in torch's own NCHW layout;
  (b) what the package could do before this kernel: ops.conv2d with pad = T // 2 on BOTH axes and a crop of the 2 (T // 2) extra rows or
      columns.
The backward baselines are one autograd.grad call giving dx AND dw, so they are set against dgrad + wgrad.

Then one Learner.train1minibatch of ImageClassificationNet(inceptionv4()) at 299 x 299 (--model-bs, 0 to skip).  The same module tree
computed by ATen is not timed here: that half of the tool ended in a segmentation fault on the GPU and was taken out until its cause is
known.  Nothing gates on these numbers.
Usage: python tools/bench_lineconv.py [--bs 32] [--iters 10] [--model-bs 32] [--skip-shapes]"""
import argparse
import os
import statistics
import sys
import time
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import ops  # noqa: E402
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402
from tools.bench_dwconv import block_us  # noqa: E402

HBM_TBS, MFMA_TFLOPS = 6.29, 157.3
# (where, C, K, map, T)
SHAPES = [('Mixed_4a', 64, 64, 73, 7), ('Inception_B', 192, 192, 17, 7), ('Inception_B', 192, 224, 17, 7), ('Inception_B', 224, 224, 17, 7),
          ('Inception_B', 224, 256, 17, 7), ('Reduction_B', 256, 256, 17, 7), ('Reduction_B', 256, 320, 17, 7),
          ('Inception_C', 384, 256, 8, 3), ('Inception_C', 384, 448, 8, 3), ('Inception_C', 448, 512, 8, 3), ('Inception_C', 512, 256, 8, 3)]


def alternate(fns, iters):
    "[(median, min, max)] in us per contender over three alternations after a warm-up of every contender"
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    blocks = [[] for _ in fns]
    for _ in range(3):
        for b, fn in zip(blocks, fns):
            b.append(block_us(fn, iters))
    return [(statistics.median(b), min(b), max(b)) for b in blocks]


def fmt(t):
    return '%8.1f (%.1f - %.1f)' % t


def bench_shapes(bs, iters):
    dev = 'cuda'
    print('%-34s %-6s | %-26s | %8s %-5s %7s | %-26s | %-26s' % ('line conv (bs %d)' % bs, 'kernel', 'us: median (min - max)', 'bound us', 'binds',
                                                              'x bound', '(a) ATen conv2d', '(b) ops.conv2d pad both + crop'))
    for where, C, K, S, T in SHAPES:
        for axis in (1, 0):
            p = T // 2
            ksz, pad = ((1, T), (0, p)) if axis else ((T, 1), (p, 0))
            x, dy = torch.randn(bs, S, S, C, device=dev), torch.randn(bs, S, S, K, device=dev)
            w = torch.randn(K, T, C, device=dev) / (T * C) ** 0.5
            wt = w.permute(2, 1, 0).contiguous()                               # W^T [C, T, K] of the dgrad
            y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
            dims = (bs, S, S, C, K, T, axis)
            wsb = int(lib.nnl_lineconv2d_wgrad_workspace_bytes(*dims))
            ws = torch.empty(max(wsb // 4, 1), device=dev)
            # (a): torch's own layouts; (b): the package's channels_last operands
            w4 = w.reshape((K,) + ksz + (C,)).permute(0, 3, 1, 2)
            xa, wa, dya = (t.contiguous().requires_grad_(g) for t, g in ((x.permute(0, 3, 1, 2), True), (w4, True), (dy.permute(0, 3, 1, 2), False)))
            xb, wb = x.permute(0, 3, 1, 2).requires_grad_(True), w4.detach().requires_grad_(True)
            dyb = dy.permute(0, 3, 1, 2)
            crop = (slice(None), slice(None), slice(p, -p), slice(None)) if axis else (slice(None), slice(None), slice(None), slice(p, -p))
            fwd_a = lambda: F.conv2d(xa, wa, None, 1, pad)                      # noqa: E731
            fwd_b = lambda: ops.conv2d(xb, wb, None, 1, p)[crop]                # noqa: E731
            ya, yb = fwd_a(), fwd_b()
            assert tuple(ya.shape) == tuple(yb.shape) == (bs, K, S, S)
            flop_us = 2.0 * bs * S * S * T * C * K / (MFMA_TFLOPS * 1e6)
            byte_us = 4.0 * (bs * S * S * (C + K) + K * T * C) / (HBM_TBS * 1e6)
            bound, binds = max(flop_us, byte_us), ('flop' if flop_us >= byte_us else 'bytes')
            ours = {
                'fwd': lambda: check(lib.nnl_lineconv2d_fwd(ptr(x), ptr(w), None, ptr(y), *dims, 0, 0, stream())),
                'dgrad': lambda: check(lib.nnl_lineconv2d_fwd(ptr(dy), ptr(wt), None, ptr(dx), bs, S, S, K, C, T, axis, 1, 0, stream())),
                'wgrad': lambda: check(lib.nnl_lineconv2d_wgrad(ptr(x), ptr(dy), ptr(dw), ptr(ws), wsb, *dims, stream())),
            }
            bwd_a = lambda: torch.autograd.grad(ya, (xa, wa), dya, retain_graph=True)      # noqa: E731
            bwd_b = lambda: torch.autograd.grad(yb, (xb, wb), dyb, retain_graph=True)      # noqa: E731
            name = '%s %d->%d %d^2 %dx%d' % ((where, C, K, S) + ksz)
            back = 0.0
            for kern in ('fwd', 'dgrad', 'wgrad'):
                t, ta, tb = alternate([ours[kern]] + ([fwd_a, fwd_b] if kern == 'fwd' else [bwd_a, bwd_b]), iters)
                back += t[0] if kern != 'fwd' else 0.0
                base = '%s | %s' % (fmt(ta), fmt(tb)) if kern != 'dgrad' else '(dx + dw: see wgrad)'
                print('%-34s %-6s | %-26s | %8.1f %-5s %7.2f | %s' % (name, kern, fmt(t), bound, binds, t[0] / bound, base), flush=True)
            print('%-34s %-6s | %8.1f' % ('', 'dg+wg', back))


def bench_model(bs, sz=299):
    from neuralnetworklibrary_amd.Applications import Vision as V
    from neuralnetworklibrary_amd.Applications.VisionModels import vmods
    from neuralnetworklibrary_amd.General.Learner import Learner
    Learner.verbose = False
    x, y = torch.randn(bs, 3, sz, sz, device='cuda'), torch.randint(0, 120, (bs,), device='cuda')
    data = types.SimpleNamespace(sz=(sz, sz), categories={i: str(i) for i in range(120)}, bs=bs, target_type='single_label')
    data.train_dl = [(None, torch.zeros(bs))]
    data.val_dl = data.train_dl
    torch.manual_seed(0)
    model = V.ImageClassificationNet(data, vmods.inceptionv4()).cuda()
    learner = Learner('/tmp/nnl_bench_lineconv', data, model, optimizer='SGD_Mom')
    learner.init_optimizer(wd=1e-4)
    lr = [1e-4] * len(model.layer_groups)
    ts = []
    for i in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = learner.train1minibatch(x, y, lr)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    steady = ts[2:]
    print('inceptionv4 train1minibatch bs %d at %d, body on the HIP kernels: median %.1f ms (min %.1f, max %.1f) over %d steps after 2 warm-up '
          'steps (loss %.4f)' % (bs, sz, statistics.median(steady), min(steady), max(steady), len(steady), loss), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--model-bs', type=int, default=32)
    ap.add_argument('--skip-shapes', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_lineconv.py measures on the GPU: none is visible')
    if not a.skip_shapes:
        bench_shapes(a.bs, a.iters)
    if a.model_bs:
        bench_model(a.model_bs)
