"""Grouped 3x3 convolution (csrc/gconv.hip) at the four stage shapes of se_resnext50_32x4d and of senet154, bs 64 at 224 x 224:
forward, dgrad and wgrad through the C ABI (no autograd / Python overhead between the launches).

Per kernel: time per launch by HIP events — after a warm-up, three alternations of (ours, the baseline), each a block of `--iters`
launches; the median of the three blocks and their spread (max - min) — that time against the larger of the traffic bound (activations
in + out once, filter once, at 6.29 TB/s) and the flop bound (157.3 TFLOP/s fp32), and against torch.nn.functional.conv2d(groups=G) on
the same device: ATen's library path, used in this tool only and never in the package.  Its input is torch's own NCHW layout; the
backward baseline is one autograd.grad call giving dx AND dw, so it is set against dgrad + wgrad.
Then one Learner.train1minibatch of ImageClassificationNet(senet154) at 224 x 224, frozen and unfrozen (--model-bs, 0 to skip).
Usage: python tools/bench_gconv.py [--bs 64] [--iters 20] [--model-bs 16] [--skip-shapes]"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402

HBM_TBS, FP32_TFLOPS = 6.29, 157.3
# (name, C, K, G, H): the steady-state 3x3 / stride 1 grouped convolution of each stage
SHAPES = [('se_resnext50 layer%d' % (i + 1), 128 << i, 128 << i, 32, 56 >> i) for i in range(4)] + \
         [('senet154 layer%d' % (i + 1), 128 << i, 256 << i, 64, 56 >> i) for i in range(4)]


def block_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def alternate(ours, base, iters):
    "((median, spread) of ours, (median, spread) of the baseline) in us over three alternations after a warm-up"
    for fn in (ours, base):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(3):
        a.append(block_us(ours, iters))
        b.append(block_us(base, iters))
    return (statistics.median(a), max(a) - min(a)), (statistics.median(b), max(b) - min(b))


def bench_shapes(bs, iters):
    dev = 'cuda'
    print('%-22s %-6s | %9s %7s | %9s %7s | %11s %7s' % ('shape (bs %d)' % bs, 'kernel', 'us', 'spread', 'bound us', 'x bound', 'ATen us', 'spread'))
    for name, C, K, G, H in SHAPES:
        Cg = C // G
        x = torch.randn(bs, H, H, C, device=dev)
        w = torch.randn(K, 3, 3, Cg, device=dev) / (9 * Cg) ** 0.5
        y, dy = torch.empty(bs, H, H, K, device=dev), torch.randn(bs, H, H, K, device=dev)
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        dims = (bs, H, H, C, K, G, 3, 1, 1)
        wsb = int(lib.nnl_gconv2d_workspace_bytes(*dims))
        ws = torch.empty(max(wsb // 4, 1), device=dev)
        xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)           # ATen's own layout
        wt = w.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        dyt = dy.permute(0, 3, 1, 2).contiguous()
        yt = F.conv2d(xt, wt, None, 1, 1, 1, G)
        flop = 2.0 * bs * H * H * K * 9 * Cg
        act = 4.0 * bs * H * H * (C + K)
        bound = max((act + 4.0 * w.numel()) / (HBM_TBS * 1e6), flop / (FP32_TFLOPS * 1e6))
        ours = {
            'fwd': lambda: check(lib.nnl_gconv2d_fwd(ptr(x), ptr(w), None, ptr(y), *dims, 0, stream())),
            'dgrad': lambda: check(lib.nnl_gconv2d_dgrad(ptr(dy), ptr(w), ptr(dx), *dims, stream())),
            'wgrad': lambda: check(lib.nnl_gconv2d_wgrad(ptr(x), ptr(dy), ptr(dw), ptr(ws), wsb, *dims, stream())),
        }
        base_fwd = lambda: F.conv2d(xt, wt, None, 1, 1, 1, G)                  # noqa: E731
        base_bwd = lambda: torch.autograd.grad(yt, (xt, wt), dyt, retain_graph=True)      # noqa: E731
        bwd_sum = 0.0
        for kern in ('fwd', 'dgrad', 'wgrad'):
            (t, sp), (tb, spb) = alternate(ours[kern], base_fwd if kern == 'fwd' else base_bwd, iters)
            bwd_sum += t if kern != 'fwd' else 0.0
            base = '%11.1f %7.1f' % (tb, spb) if kern != 'dgrad' else '%11s %7s' % ('(see wgrad)', '')
            print('%-22s %-6s | %9.1f %7.1f | %9.1f %7.2f | %s' % ('%s %dx%d g%d %d' % (name, Cg, K // G, G, H), kern, t, sp, bound, t / bound, base))
        print('%-22s %-6s | %9.1f' % ('', 'dg+wg', bwd_sum))


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
    model = V.ImageClassificationNet(data, vmods.senet154()).cuda()
    learner = Learner('/tmp/nnl_bench_gconv', data, model, optimizer='SGD_Mom')
    learner.init_optimizer(wd=1e-4)
    x, y = torch.randn(bs, 3, 224, 224, device='cuda'), torch.randint(0, 120, (bs,), device='cuda')
    lr = [1e-4] * len(model.layer_groups)
    for what in ('frozen', 'unfrozen'):
        if what == 'frozen':
            learner.freeze()
            learner.bn_freeze()
        else:
            learner.unfreeze()
            learner.bn_unfreeze()
        ts = []
        for i in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = learner.train1minibatch(x, y, lr)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        steady = ts[2:]
        print('senet154 train1minibatch bs %d at 224, %-8s: median %.1f ms, spread %.1f ms over %d steps after 2 warm-up steps (loss %.4f)'
              % (bs, what, statistics.median(steady), max(steady) - min(steady), len(steady), loss), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--model-bs', type=int, default=16)
    ap.add_argument('--skip-shapes', action='store_true')
    a = ap.parse_args()
    if not a.skip_shapes:
        bench_shapes(a.bs, a.iters)
    if a.model_bs:
        bench_model(a.model_bs)
