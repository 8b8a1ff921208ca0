"""bf16 matrix-core convolutions (csrc/conv_bf16.hip) against today's fp32 route at the distinct body-convolution geometries of ResNet-34
(bs 64, 224 x 224) and of RetinaNet-R50 (bs 16, 512 x 512: the backbone's bottlenecks and the 256-channel 3x3 of the pyramid and the
heads), through the C ABI (no autograd / Python overhead between the launches).

Per direction: time per launch by HIP events — after a warm-up, three alternations of (bf16, fp32), each a block of `--iters` launches;
the median of the three blocks with min - max — against max(flop over the 2516.6 TFLOP/s bf16 peak, the fp32 tensors of the call read or
written once over 6.29 TB/s).  The bf16 forward and dgrad INCLUDE their filter pack launch (ops.conv2d_bf16 packs per call); the fp32
dgrad EXCLUDES its filter transpose (the prepared-filter window batches those once per step) and both fp32 calls get their workspace and
tile counters, so they take the Winograd / balanced kernels exactly as in training.  Before a geometry is timed, the two routes' outputs
are compared at the timed size (the difference is the bf16 rounding of the operands: about 2^-9 per operand, relative to sum|terms|).
Then Learner.train1minibatch of ResNet-34 at bs 64 (--model-bs, 0 to skip) with and without use_bf16_conv(), alternated three times.
Usage: python tools/bench_conv_bf16.py [--iters 10] [--model-bs 64] [--skip-shapes]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import ops  # noqa: E402
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402

HBM_TBS, BF16_TFLOPS = 6.29, 2516.6


def shapes():
    "(name, bs, C, K, R, stride, H): distinct geometries only"
    out = [('r34 layer1 3x3', 64, 64, 64, 3, 1, 56)]
    for i in range(1, 4):
        c, h = 64 << i, 56 >> i
        out += [('r34 layer%d 3x3/2' % (i + 1), 64, c // 2, c, 3, 2, 2 * h), ('r34 layer%d 1x1/2' % (i + 1), 64, c // 2, c, 1, 2, 2 * h),
                ('r34 layer%d 3x3' % (i + 1), 64, c, c, 3, 1, h)]
    for i in range(4):
        p, h, cin = 64 << i, 128 >> i, (64 if i == 0 else 128 << i)          # planes, the stage's map, the channels that enter it
        hin, s = (h, 1) if i == 0 else (2 * h, 2)
        out += [('r50 layer%d 1x1 in' % (i + 1), 16, cin, p, 1, 1, hin), ('r50 layer%d 3x3%s' % (i + 1, '/2' if s == 2 else ''), 16, p, p, 3, s, hin),
                ('r50 layer%d 1x1 out' % (i + 1), 16, p, 4 * p, 1, 1, h), ('r50 layer%d proj' % (i + 1), 16, cin, 4 * p, 1, s, hin),
                ('r50 layer%d 1x1 back' % (i + 1), 16, 4 * p, p, 1, 1, h)]
        if s == 2:
            out.append(('r50 layer%d 3x3' % (i + 1), 16, p, p, 3, 1, h))
    out += [('fpn / heads 3x3 at %d' % h, 16, 256, 256, 3, 1, h) for h in (64, 32, 16, 8, 4)]
    return out


def block_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def alternate(ours, base, iters):
    "((median, min, max) of ours, of the baseline) in us over three alternations after a warm-up"
    for fn in (ours, base):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(3):
        a.append(block_us(ours, iters))
        b.append(block_us(base, iters))
    return (statistics.median(a), min(a), max(a)), (statistics.median(b), min(b), max(b))


def bench_shapes(iters):
    dev = 'cuda'
    counters = torch.zeros(int(lib.nnl_conv2d_tile_counters()), dtype=torch.int32, device=dev)
    print('%-26s %-5s | %8s %17s | %8s %17s | %7s | %8s %7s' % ('geometry', 'dir', 'bf16 us', 'min - max', 'fp32 us', 'min - max', 'fp32/bf', 'bound us', 'x bound'))
    for name, bs, C, K, R, stride, H in shapes():
        pad = R // 2
        g = ops._geom(bs, H, H, C, K, R, R, stride, pad)
        assert lib.nnl_conv2d_bf16_supported(g), name
        x, dy = torch.randn(bs, H, H, C, device=dev), torch.randn(bs, g.P, g.Q, K, device=dev)
        w = torch.randn(K, R, R, C, device=dev) / (R * R * C) ** 0.5
        wt = torch.empty(C, R, R, K, device=dev)
        check(lib.nnl_conv2d_weight_transpose(ptr(w), ptr(wt), K, R, R, C, stream()))
        wp = torch.empty(w.numel(), dtype=torch.bfloat16, device=dev)
        outs = {k: (torch.empty_like(t), torch.empty_like(t)) for k, t in (('fwd', dy), ('dgrad', x), ('wgrad', w))}
        wsb = {k: int(f(g)) for k, f in (('fwd', lib.nnl_conv2d_fwd_workspace_bytes), ('dgrad', lib.nnl_conv2d_dgrad_workspace_bytes),
                                         ('wgrad', lib.nnl_conv2d_wgrad_workspace_bytes), ('wgrad16', lib.nnl_conv2d_bf16_wgrad_workspace_bytes))}
        ws = {k: torch.empty(max(v // 4, 1), device=dev) for k, v in wsb.items()}
        cnt = lambda k: ptr(counters) if wsb[k] else None                       # noqa: E731

        def bf16(kind, out):
            if kind == 'fwd':
                check(lib.nnl_conv2d_bf16_pack_filter(ptr(w), ptr(wp), g, 0, stream()))
                check(lib.nnl_conv2d_bf16_fwd(ptr(x), ptr(wp), None, ptr(out), g, 0, stream()))
            elif kind == 'dgrad':
                check(lib.nnl_conv2d_bf16_pack_filter(ptr(w), ptr(wp), g, 1, stream()))
                check(lib.nnl_conv2d_bf16_dgrad(ptr(dy), ptr(wp), ptr(out), g, None, stream()))
            else:
                check(lib.nnl_conv2d_bf16_wgrad(ptr(x), ptr(dy), ptr(out), g, ptr(ws['wgrad16']), wsb['wgrad16'], stream()))

        def fp32(kind, out):
            if kind == 'fwd':
                check(lib.nnl_conv2d_fwd_pre(ptr(x), ptr(w), None, ptr(out), g, 0, ptr(ws['fwd']) if wsb['fwd'] else None, wsb['fwd'], cnt('fwd'),
                                             None, None, None, None, stream()))
            elif kind == 'dgrad':
                check(lib.nnl_conv2d_dgrad_pre(ptr(dy), ptr(wt), ptr(out), g, None, ptr(ws['dgrad']) if wsb['dgrad'] else None, wsb['dgrad'],
                                               cnt('dgrad'), None, stream()))
            else:
                check(lib.nnl_conv2d_wgrad(ptr(x), ptr(dy), ptr(out), g, ptr(ws['wgrad']), wsb['wgrad'], stream()))
        flop = 2.0 * bs * g.P * g.Q * K * R * R * C
        bound = max(flop / (BF16_TFLOPS * 1e6), 4.0 * (x.numel() + dy.numel() + w.numel()) / (HBM_TBS * 1e6))
        for kind in ('fwd', 'dgrad', 'wgrad'):
            o16, o32 = outs[kind]
            bf16(kind, o16)
            fp32(kind, o32)
            rel = ((o16 - o32).abs().max() / o32.abs().max()).item()
            assert rel < 0.05, '%s %s: the two routes differ by %.3f of the largest value' % (name, kind, rel)
            (t, lo, hi), (tb, lob, hib) = alternate(lambda: bf16(kind, o16), lambda: fp32(kind, o32), iters)
            print('%-26s %-5s | %8.1f %8.1f-%8.1f | %8.1f %8.1f-%8.1f | %7.2f | %8.1f %7.2f' % (
                '%s %d>%d @%d bs%d' % (name, C, K, H, bs), kind, t, lo, hi, tb, lob, hib, tb / t, bound, t / bound), flush=True)


def bench_model(bs):
    import types

    from neuralnetworklibrary_amd.Applications import Vision as V
    from neuralnetworklibrary_amd.Applications.VisionModels import vmods
    from neuralnetworklibrary_amd.General.Learner import Learner
    Learner.verbose = False
    data = types.SimpleNamespace(sz=(224, 224), categories={i: str(i) for i in range(120)}, bs=bs, target_type='single_label')
    data.train_dl = [(None, torch.zeros(bs))]
    data.val_dl = data.train_dl
    torch.manual_seed(0)
    model = V.ImageClassificationNet(data, vmods.resnet34()).cuda()
    learner = Learner('/tmp/nnl_bench_conv_bf16', data, model, optimizer='SGD_Mom')
    learner.init_optimizer(wd=1e-4)
    learner.unfreeze()
    x, y = torch.randn(bs, 3, 224, 224, device='cuda'), torch.randint(0, 120, (bs,), device='cuda')
    lr = [1e-4] * len(model.layer_groups)

    def steps(flag, n):
        learner.use_bf16_conv(flag)
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            learner.train1minibatch(x, y, lr)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts[2:]                                                     # two warm-up steps after every switch
    res = {True: [], False: []}
    for _ in range(3):
        for flag in (True, False):
            ts = steps(flag, 8)
            res[flag].append(statistics.median(ts))
    for flag in (True, False):
        print('resnet34 train1minibatch bs %d at 224, %s convolutions: median %.1f ms (min %.1f - max %.1f over three alternations of 6 steps)'
              % (bs, 'bf16' if flag else 'fp32', statistics.median(res[flag]), min(res[flag]), max(res[flag])), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--model-bs', type=int, default=64)
    ap.add_argument('--skip-shapes', action='store_true')
    a = ap.parse_args()
    if not a.skip_shapes:
        bench_shapes(a.iters)
    if a.model_bs:
        bench_model(a.model_bs)
