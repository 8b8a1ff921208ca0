"""bf16 matrix-core grouped convolutions (csrc/gconv_bf16.hip) against today's fp32 route (csrc/gconv.hip: the direct kernels at 4 and 8
channels per group, the fp32 MFMA kernels of gconv_mfma.h at 16 and 32) at every grouped shape of the zoo inside the bf16 domain, bs 64 at
224 x 224: resnext101_32x4d / se_resnext50 / se_resnext101 (G 32), resnext101_64x4d (G 64) and senet154 (G 64, Kg = 2 Cg), through the C ABI
(no autograd / Python overhead between the launches).

The protocol of tools/bench_conv_bf16.py.  Per direction: time per launch by HIP events — after a warm-up, three alternations of (bf16,
fp32), each a block of `--iters` launches; the median of the three blocks with min - max — against max(flop over the 2516.6 TFLOP/s bf16
peak, the fp32 tensors of the call read or written once over 6.29 TB/s).  Both wgrads include their fold launch.  Before a geometry is
timed, the two routes' outputs are compared at the timed size (the difference is the bf16 rounding of the operands).
Then Learner.train1minibatch of resnext101_32x4d at bs 64 (--model-bs, 0 to skip), unfrozen, SGD with momentum, under three settings
alternated three times, the median of 3 steps after 2 warm-up steps each: use_bf16_conv() with the grouped modules kept on fp32 (the mode
as it was before this kernel family), use_bf16_conv() as it is, and all fp32.
Usage: python tools/bench_gconv_bf16.py [--iters 10] [--model-bs 64] [--skip-shapes]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_conv_bf16 import BF16_TFLOPS, HBM_TBS, alternate  # noqa: E402
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402


def shapes():
    "(name, C, K, G, stride, H): the grouped 3x3 of every stage, and the stride-2 one that opens stages 2 - 4"
    out = []
    for name, G in (('32x4d', 32), ('64x4d', 64)):
        for i in range(4):
            c, h = 4 * G << i, 56 >> i
            if i:
                out.append(('%s layer%d /2' % (name, i + 1), c, c, G, 2, 2 * h))
            out.append(('%s layer%d' % (name, i + 1), c, c, G, 1, h))
    for i in range(1, 4):                                                     # (layer1 has 2 channels per group: outside the domain)
        c, h = 128 << i, 56 >> i
        out += [('senet154 layer%d /2' % (i + 1), c, 2 * c, 64, 2, 2 * h), ('senet154 layer%d' % (i + 1), c, 2 * c, 64, 1, h)]
    return out


def bench_shapes(bs, iters):
    dev = 'cuda'
    print('%-34s %-5s | %8s %17s | %8s %17s | %7s | %8s %7s' % ('geometry', 'dir', 'bf16 us', 'min - max', 'fp32 us', 'min - max', 'fp32/bf', 'bound us', 'x bound'))
    for name, C, K, G, stride, H in shapes():
        R, pad = 3, 1
        dims = (bs, H, H, C, K, G, R, stride, pad)
        assert lib.nnl_gconv2d_bf16_supported(*dims), name
        P = (H + 2 * pad - R) // stride + 1
        x, dy = torch.randn(bs, H, H, C, device=dev), torch.randn(bs, P, P, K, device=dev)
        w = torch.randn(K, R, R, C // G, device=dev) / (R * R * C // G) ** 0.5
        outs = {k: (torch.empty_like(t), torch.empty_like(t)) for k, t in (('fwd', dy), ('dgrad', x), ('wgrad', w))}
        wsb = {'bf16': int(lib.nnl_gconv2d_bf16_workspace_bytes(*dims)), 'fp32': int(lib.nnl_gconv2d_workspace_bytes(*dims))}
        ws = {k: torch.empty(max(v // 4, 1), device=dev) for k, v in wsb.items()}

        def run(route, kind, out):
            pre = 'nnl_gconv2d_bf16_' if route == 'bf16' else 'nnl_gconv2d_'
            if kind == 'fwd':
                check(getattr(lib, pre + 'fwd')(ptr(x), ptr(w), None, ptr(out), *dims, 0, stream()))
            elif kind == 'dgrad':
                check(getattr(lib, pre + 'dgrad')(ptr(dy), ptr(w), ptr(out), *dims, stream()))
            else:
                check(getattr(lib, pre + 'wgrad')(ptr(x), ptr(dy), ptr(out), ptr(ws[route]), wsb[route], *dims, stream()))
        flop = 2.0 * bs * P * P * K * R * R * (C // G)
        bound = max(flop / (BF16_TFLOPS * 1e6), 4.0 * (x.numel() + dy.numel() + w.numel()) / (HBM_TBS * 1e6))
        for kind in ('fwd', 'dgrad', 'wgrad'):
            o16, o32 = outs[kind]
            run('bf16', kind, o16)
            run('fp32', kind, o32)
            rel = ((o16 - o32).abs().max() / o32.abs().max()).item()
            assert rel < 0.05, '%s %s: the two routes differ by %.3f of the largest value' % (name, kind, rel)
            (t, lo, hi), (tb, lob, hib) = alternate(lambda: run('bf16', kind, o16), lambda: run('fp32', kind, o32), iters)
            print('%-34s %-5s | %8.1f %8.1f-%8.1f | %8.1f %8.1f-%8.1f | %7.2f | %8.1f %7.2f' % (
                '%s %d/%d @%d' % (name, C // G, K // G, H), kind, t, lo, hi, tb, lob, hib, tb / t, bound, t / bound), flush=True)


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
    model = V.ImageClassificationNet(data, vmods.resnext101_32x4d()).cuda()
    learner = Learner('/tmp/nnl_bench_gconv_bf16', data, model, optimizer='SGD_Mom')
    learner.init_optimizer(wd=1e-4)
    learner.unfreeze()
    x, y = torch.randn(bs, 3, 224, 224, device='cuda'), torch.randint(0, 120, (bs,), device='cuda')
    lr = [1e-4] * len(model.layer_groups)

    def steps(setting):
        learner.use_bf16_conv(setting != 'all fp32')
        if setting == 'bf16, grouped on fp32':
            for m in model.modules():
                if getattr(m, 'nnl_hip_gconv', False):
                    m.compute = 'fp32'
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            learner.train1minibatch(x, y, lr)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[2:])                                      # two warm-up steps after every switch
    settings = ('bf16, grouped on fp32', 'bf16, grouped on bf16', 'all fp32')
    res = {k: [] for k in settings}
    for _ in range(3):
        for k in settings:
            res[k].append(steps(k))
    for k in settings:
        print('resnext101_32x4d train1minibatch bs %d at 224, %-22s: median %.1f ms (min %.1f - max %.1f over three alternations of 3 steps)'
              % (bs, k, statistics.median(res[k]), min(res[k]), max(res[k])), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=64)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--model-bs', type=int, default=64)
    ap.add_argument('--skip-shapes', action='store_true')
    a = ap.parse_args()
    if not a.skip_shapes:
        bench_shapes(a.bs, a.iters)
    if a.model_bs:
        bench_model(a.model_bs)
