"""Depthwise convolution (csrc/dwconv.hip) and average pool (csrc/pool.hip) at the geometries of NASNet-A-Large at 331 x 331, bs 16:
C in {42, 84, 96, 168, 336, 672} on the maps 165 / 83 / 42 / 21 / 11, each (R, stride) that occurs there, the stride-2 ones of
ReductionCell0 in their folded form (pad_lo = R // 2 - 1).  Forward, dgrad and wgrad through the C ABI (no autograd / Python overhead
between the launches).

Per kernel: time per launch by HIP events — after a warm-up, three alternations of (ours, the baseline), each a block of `--iters`
launches; the median of the three blocks and their spread (max - min) — that time against the traffic bound (activations read once plus
output written once, at 6.29 TB/s: the layer has no reduction over channels, at R = 7 it does 98 flop per 8 bytes moved), and against
torch.nn.functional.conv2d(groups=C) / avg_pool2d on the same device: ATen's library path, used in this tool only and never in the
package.  Its input is torch's own NCHW layout, the folded forms are the reference's pad -> op -> slice chain; the backward baseline is
one autograd.grad call giving dx AND dw, so it is set against dgrad + wgrad.

Then one Learner.train1minibatch of ImageClassificationNet(nasnetalarge()) at 331 x 331 (--model-bs, 0 to skip), next to the same
network computed by ATen: the same module tree with the `ops` namespace of its modules replaced by the ATen compositions of AtenOps
below (F.conv2d, F.batch_norm, F.avg_pool2d / F.max_pool2d, F.pad + slice), parameters in torch's own contiguous layout.  The parent of
this tool has no such model: ATen is the only baseline.  Nothing gates on these numbers.
Usage: python tools/bench_dwconv.py [--bs 16] [--iters 20] [--model-bs 16] [--skip-shapes]"""
import argparse
import contextlib
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import ops  # noqa: E402
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402

HBM_TBS = 6.29
# (where, C, H, R, stride, folded)
SHAPES = [('stem0', 96, 165, 7, 2, 0), ('stem0', 96, 165, 5, 2, 0), ('stem0', 42, 165, 5, 2, 0), ('stem0', 42, 83, 7, 1, 0),
          ('stem0', 42, 83, 5, 1, 0), ('stem0', 42, 83, 3, 1, 0), ('stem1', 84, 83, 7, 2, 0), ('stem1', 84, 83, 5, 2, 0),
          ('stem1', 84, 42, 7, 1, 0), ('stem1', 84, 42, 5, 1, 0), ('stem1', 84, 42, 3, 1, 0), ('cell0-5', 168, 42, 5, 1, 0),
          ('cell0-5', 168, 42, 3, 1, 0), ('reduc0', 336, 42, 7, 2, 1), ('reduc0', 336, 42, 5, 2, 1), ('reduc0', 336, 21, 7, 1, 0),
          ('cell6-11', 336, 21, 5, 1, 0), ('cell6-11', 336, 21, 3, 1, 0), ('reduc1', 672, 21, 7, 2, 0), ('reduc1', 672, 21, 5, 2, 0),
          ('reduc1', 672, 11, 7, 1, 0), ('cell12-17', 672, 11, 5, 1, 0), ('cell12-17', 672, 11, 3, 1, 0)]
# (where, C, H, stride, folded): AvgPool2d(3, stride, 1, count_include_pad=False)
POOLS = [('stem0', 42, 165, 2, 0), ('stem0', 42, 83, 1, 0), ('cell0-5', 168, 42, 1, 0), ('reduc0', 336, 42, 2, 1), ('cell6-11', 336, 21, 1, 0),
         ('cell12-17', 672, 11, 1, 0)]


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


def window(H, R, stride, folded):
    "(pad_lo, P) of the op, and its literal ATen form"
    p = R // 2
    return ops.fold_zero_pad(H, R, stride, p, 1) if folded else (p, (H + 2 * p - R) // stride + 1)


def bench_shapes(bs, iters):
    dev = 'cuda'
    head = '%-26s %-6s | %9s %7s | %9s %7s | %11s %7s'
    print(head % ('depthwise conv (bs %d)' % bs, 'kernel', 'us', 'spread', 'bound us', 'x bound', 'ATen us', 'spread'))
    for where, C, H, R, stride, folded in SHAPES:
        p = R // 2
        lo, P = window(H, R, stride, folded)
        x = torch.randn(bs, H, H, C, device=dev)
        w = torch.randn(C, 1, R, R, device=dev) / R
        y, dy = torch.empty(bs, P, P, C, device=dev), torch.randn(bs, P, P, C, device=dev)
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        dims = (bs, H, H, C, P, P, R, stride, lo)
        wsb = int(lib.nnl_dwconv2d_wgrad_workspace_bytes(*dims))
        ws = torch.empty(max(wsb // 4, 1), device=dev)
        xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)           # ATen's own layout
        wt = w.clone().requires_grad_(True)
        dyt = dy.permute(0, 3, 1, 2).contiguous()

        def base_fwd():
            if folded:
                return F.conv2d(F.pad(torch.relu(xt), (1, 0, 1, 0)), wt, None, stride, p, 1, C)[:, :, 1:, 1:]
            return F.conv2d(torch.relu(xt), wt, None, stride, p, 1, C)
        yt = base_fwd()
        assert tuple(yt.shape) == (bs, C, P, P)
        bound = 4.0 * bs * C * (H * H + P * P) / (HBM_TBS * 1e6)
        ours = {                                                                # relu_in = 1: how every BranchSeparables calls its first one
            'fwd': lambda: check(lib.nnl_dwconv2d_fwd(ptr(x), ptr(w), None, ptr(y), *dims, 1, stream())),
            'dgrad': lambda: check(lib.nnl_dwconv2d_dgrad(ptr(dy), ptr(w), ptr(x), ptr(dx), *dims, 1, stream())),
            'wgrad': lambda: check(lib.nnl_dwconv2d_wgrad(ptr(x), ptr(dy), ptr(dw), ptr(ws), wsb, *dims, 1, stream())),
        }
        base_bwd = lambda: torch.autograd.grad(yt, (xt, wt), dyt, retain_graph=True)      # noqa: E731
        bwd_sum = 0.0
        name = '%s C%d %d^2 %dx%d/%d%s' % (where, C, H, R, R, stride, 'f' if folded else '')
        for kern in ('fwd', 'dgrad', 'wgrad'):
            (t, sp), (tb, spb) = alternate(ours[kern], base_fwd if kern == 'fwd' else base_bwd, iters)
            bwd_sum += t if kern != 'fwd' else 0.0
            base = '%11.1f %7.1f' % (tb, spb) if kern != 'dgrad' else '%11s %7s' % ('(see wgrad)', '')
            print('%-26s %-6s | %9.1f %7.1f | %9.1f %7.2f | %s' % (name, kern, t, sp, bound, t / bound, base), flush=True)
        print('%-26s %-6s | %9.1f' % ('', 'dg+wg', bwd_sum))
    print(head % ('avg pool 3x3 (bs %d)' % bs, 'kernel', 'us', 'spread', 'bound us', 'x bound', 'ATen us', 'spread'))
    for where, C, H, stride, folded in POOLS:
        lo, P = window(H, 3, stride, folded)
        x = torch.randn(bs, H, H, C, device=dev)
        y, dy, dx = torch.empty(bs, P, P, C, device=dev), torch.randn(bs, P, P, C, device=dev), torch.empty_like(x)
        dims = (bs, H, H, C, P, P, 3, stride, lo, 0)
        xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        dyt = dy.permute(0, 3, 1, 2).contiguous()

        def base_fwd():
            if folded:
                return F.avg_pool2d(F.pad(xt, (1, 0, 1, 0)), 3, stride, 1, count_include_pad=False)[:, :, 1:, 1:]
            return F.avg_pool2d(xt, 3, stride, 1, count_include_pad=False)
        yt = base_fwd()
        assert tuple(yt.shape) == (bs, C, P, P)
        bound = 4.0 * bs * C * (H * H + P * P) / (HBM_TBS * 1e6)
        name = '%s C%d %d^2 /%d%s' % (where, C, H, stride, 'f' if folded else '')
        for kern, fn, base in (('fwd', lambda: check(lib.nnl_avgpool2d_fwd(ptr(x), ptr(y), *dims, stream())), base_fwd),
                               ('bwd', lambda: check(lib.nnl_avgpool2d_bwd(ptr(dy), ptr(dx), *dims, stream())),
                                lambda: torch.autograd.grad(yt, xt, dyt, retain_graph=True))):
            (t, sp), (tb, spb) = alternate(fn, base, iters)
            print('%-26s %-6s | %9.1f %7.1f | %9.1f %7.2f | %11.1f %7.1f' % (name, kern, t, sp, bound, t / bound, tb, spb), flush=True)


class AtenOps:
    "what the NASNet modules ask of `ops`, computed by ATen in torch's NCHW layout: the baseline network of bench_model"
    fold_zero_pad = staticmethod(ops.fold_zero_pad)
    fan_param = staticmethod(lambda p: p)

    @staticmethod
    def _unfold(pad, pad_lo, stride):
        "the top/left zero padding whose folding gave pad_lo (ops.fold_zero_pad): None for the plain op"
        return None if pad_lo is None else pad_lo - pad + stride

    @staticmethod
    def conv2d(x, weight, bias=None, stride=1, pad=0, relu=False, grad_slot=None, give_slot=None):
        y = F.conv2d(x, weight, bias, stride, pad)
        return F.relu(y) if relu else y

    @staticmethod
    def depthwise_conv2d(x, weight, bias, stride, pad, pad_lo=None, out_size=None, relu_in=False):
        a, z = (F.relu(x) if relu_in else x), AtenOps._unfold(pad, pad_lo, stride)
        if z is None:
            return F.conv2d(a, weight, bias, stride, pad, 1, x.shape[1])
        return F.conv2d(F.pad(a, (z, 0, z, 0)), weight, bias, stride, pad, 1, x.shape[1])[:, :, 1:, 1:].contiguous()

    @staticmethod
    def avgpool2d(x, ksize, stride, pad, count_include_pad=True, pad_lo=None, out_size=None):
        z = AtenOps._unfold(pad, pad_lo, stride)
        if z is None:
            return F.avg_pool2d(x, ksize, stride, pad, count_include_pad=count_include_pad)
        return F.avg_pool2d(F.pad(x, (z, 0, z, 0)), ksize, stride, pad, count_include_pad=count_include_pad)[:, :, 1:, 1:]

    @staticmethod
    def subsample2d(x, stride, off):
        return F.avg_pool2d(F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:] if off else x, 1, stride)

    @staticmethod
    def maxpool2d(x, ksize=3, stride=2, pad=1, ceil_mode=False):
        if ceil_mode:                                                           # MaxPoolPad, as the reference writes it
            return F.max_pool2d(F.pad(x, (1, 0, 1, 0)), 3, 2, 1)[:, :, 1:, 1:]
        return F.max_pool2d(x, ksize, stride, pad)

    @staticmethod
    def bn_act(bn, x, residual=None, relu=True, **kw):
        y = torch.nn.BatchNorm2d.forward(bn, x)
        return F.relu(y) if relu else y

    @staticmethod
    def conv_bn_act(conv, bn, x, residual=None, relu=True, **kw):
        return AtenOps.bn_act(bn, F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding), relu=relu)


@contextlib.contextmanager
def aten_body():
    from neuralnetworklibrary_amd.Applications.VisionModels import nasnet, retinanet
    saved = nasnet.ops, retinanet.ops
    nasnet.ops = retinanet.ops = AtenOps
    try:
        yield
    finally:
        nasnet.ops, retinanet.ops = saved


def bench_model(bs, sz=331):
    import types

    from neuralnetworklibrary_amd.Applications import Vision as V
    from neuralnetworklibrary_amd.Applications.VisionModels import vmods
    from neuralnetworklibrary_amd.General.Learner import Learner
    Learner.verbose = False
    x, y = torch.randn(bs, 3, sz, sz, device='cuda'), torch.randint(0, 120, (bs,), device='cuda')
    for what in ('hip', 'aten'):
        with (aten_body() if what == 'aten' else contextlib.nullcontext()):
            data = types.SimpleNamespace(sz=(sz, sz), categories={i: str(i) for i in range(120)}, bs=bs, target_type='single_label')
            data.train_dl = [(None, torch.zeros(bs))]
            data.val_dl = data.train_dl
            torch.manual_seed(0)
            model = V.ImageClassificationNet(data, vmods.nasnetalarge()).cuda()
            if what == 'aten':
                for p in model.body.parameters():
                    p.data = p.data.contiguous()
            learner = Learner('/tmp/nnl_bench_dwconv', data, model, optimizer='SGD_Mom')
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
            print('nasnetalarge train1minibatch bs %d at %d, body on %-4s: median %.1f ms, spread %.1f ms over %d steps after 2 warm-up steps '
                  '(loss %.4f)' % (bs, sz, what, statistics.median(steady), max(steady) - min(steady), len(steady), loss), flush=True)
            del learner, model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--model-bs', type=int, default=16)
    ap.add_argument('--skip-shapes', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_dwconv.py measures on the GPU: none is visible')
    if not a.skip_shapes:
        bench_shapes(a.bs, a.iters)
    if a.model_bs:
        bench_model(a.model_bs)
