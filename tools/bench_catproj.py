"""Concat-fused residual projection (csrc/catproj.hip, K20) at the three residual-block shapes of InceptionResNetV2 at 299 x 299, bs 32:
Block35 (35 x 35, sources 32 + 32 + 64 -> 320, scale 0.17), Block17 (17 x 17, 192 + 192 -> 1088, 0.10), Block8 (8 x 8, 192 + 256 -> 2080, 0.20).
Forward, dgrad and wgrad through the C ABI (no autograd / Python overhead between the launches).

Per kernel: time per launch by HIP events — after a warm-up of every contender, three alternations of (ours, baseline a, baseline b) in
one process, each a block of `--iters` launches; the median of the three blocks with min and max — and that time against the bound
max(2 M Ctot K / 157.3 TFLOP/s, bytes touched once / 6.29 TB/s) computed from the shapes here, with the side that binds named.
The baselines live in this tool only:
  (a) what the package offered before this kernel: torch.cat -> ops.conv2d (1 x 1, bias) -> out * scale + x -> relu, and its backward;
  (b) the same in plain ATen (F.conv2d), one layer at a time.
The backward baselines are one autograd.grad call giving every source gradient, dw, db and the residual's gradient, so they are set
against dgrad + wgrad.  Before anything is timed the outputs of the fused route and of (a) are compared at the timed size, in ulps of the
largest value.

Then one Learner.train1minibatch of ImageClassificationNet(inceptionresnetv2()) at 299 x 299 (--model-bs, 0 to skip): with the blocks on
the fused op, and — in processes of their own — with the blocks' forward replaced here by route (a) (`--route a`) and with the routes
the model ships with (`--route model`).  Nothing gates on these
numbers; README "InceptionResNetV2" states the rule by which a block class keeps the fused op.
Usage: python tools/bench_catproj.py [--bs 32] [--iters 10] [--model-bs 32] [--skip-shapes] [--route fused|a|model]"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import ops  # noqa: E402
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402
from tools.bench_lineconv import HBM_TBS, MFMA_TFLOPS, alternate, fmt  # noqa: E402

# (where, map, sources, K, scale)
SHAPES = [('Block35', 35, (32, 32, 64), 320, 0.17), ('Block17', 17, (192, 192), 1088, 0.10), ('Block8', 8, (192, 256), 2080, 0.20)]


def route_a(conv, xs, x, scale, relu, conv2d=ops.conv2d):
    out = conv2d(torch.cat(xs, 1), conv.weight, conv.bias) * scale + x
    return torch.relu(out) if relu else out


def bench_shapes(bs, iters):
    dev = 'cuda'
    print('%-28s %-6s | %-26s | %8s %-5s %7s | %-26s | %-26s' % ('residual tail (bs %d)' % bs, 'kernel', 'us: median (min - max)', 'bound us', 'binds',
                                                               'x bound', '(a) cat + ops.conv2d + ATen', '(b) ATen'))
    for where, S, sources, K, scale in SHAPES:
        M, Ctot, n = bs * S * S, sum(sources), len(sources)
        xs = [torch.randn(bs, S, S, c, device=dev) for c in sources]
        res, dy = torch.randn(bs, S, S, K, device=dev), torch.randn(bs, S, S, K, device=dev)
        w, b = torch.randn(K, Ctot, device=dev) / Ctot ** 0.5, torch.randn(K, device=dev)
        y, dres, dw = torch.empty_like(res), torch.empty_like(res), torch.empty_like(w)
        dxs = [torch.empty_like(x) for x in xs]
        ch = (ctypes.c_int64 * n)(*sources)
        pa = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
        wsb = int(lib.nnl_catproj_wgrad_workspace_bytes(ch, n, M, K))
        ws = torch.empty(max(wsb // 4, 1), device=dev)
        ours = {
            'fwd': lambda: check(lib.nnl_catproj_fwd(pa(xs), ch, n, ptr(w), ptr(b), ptr(res), ptr(y), M, K, scale, 1, stream())),
            'dgrad': lambda: check(lib.nnl_catproj_dgrad(ptr(dy), ptr(y), ptr(w), pa(dxs), ch, n, ptr(dres), M, K, scale, 1, stream())),
            'wgrad': lambda: check(lib.nnl_catproj_wgrad(pa(xs), ch, n, ptr(dres), None, ptr(dw), ptr(ws), wsb, M, K, scale, 0, stream())),
        }
        conv = types.SimpleNamespace(weight=w.view(K, Ctot, 1, 1).requires_grad_(True), bias=b.clone().requires_grad_(True))
        la = [t.permute(0, 3, 1, 2).requires_grad_(True) for t in xs + [res]]                 # channels_last, the package's layout
        lb = [t.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in xs + [res]]    # torch's own NCHW
        dya, dyb = dy.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2).contiguous()
        fwd_a = lambda: route_a(conv, la[:n], la[n], scale, True)                # noqa: E731
        fwd_b = lambda: route_a(conv, lb[:n], lb[n], scale, True, F.conv2d)      # noqa: E731
        ya, yb = fwd_a(), fwd_b()
        ours['fwd']()
        dist = (y.permute(0, 3, 1, 2) - ya).abs().max().item()
        big = max(y.abs().max().item(), 1e-30)
        print('%-28s fused vs (a): max |difference| %.3e = %.1f ulp of the largest value %.3f' % (where, dist, dist / (big * 2.0 ** -23), big), flush=True)
        bwd_a = lambda: torch.autograd.grad(ya, la + [conv.weight, conv.bias], dya, retain_graph=True)      # noqa: E731
        bwd_b = lambda: torch.autograd.grad(yb, lb + [conv.weight, conv.bias], dyb, retain_graph=True)      # noqa: E731
        flop_us = 2.0 * M * Ctot * K / (MFMA_TFLOPS * 1e6)
        byte_us = 4.0 * (M * (Ctot + 2 * K) + K * Ctot) / (HBM_TBS * 1e6)
        bound, binds = max(flop_us, byte_us), ('flop' if flop_us >= byte_us else 'bytes')
        name = '%s %s->%d %d^2' % (where, '+'.join(map(str, sources)), K, S)
        total = {'ours': [0.0, 0.0], 'a': [0.0, 0.0]}
        for kern in ('fwd', 'dgrad', 'wgrad'):
            t, ta, tb = alternate([ours[kern]] + ([fwd_a, fwd_b] if kern == 'fwd' else [bwd_a, bwd_b]), iters)
            total['ours'][0] += t[0]
            total['ours'][1] += t[2] - t[1]
            if kern != 'dgrad':
                total['a'][0] += ta[0]
                total['a'][1] += ta[2] - ta[1]
            base = '%s | %s' % (fmt(ta), fmt(tb)) if kern != 'dgrad' else '(all gradients: see wgrad)'
            print('%-28s %-6s | %-26s | %8.1f %-5s %7.2f | %s' % (name, kern, fmt(t), bound, binds, t[0] / bound, base), flush=True)
        print('%-28s %-6s | fused %.1f us (spreads add to %.1f), route (a) %.1f us (spreads add to %.1f)'
              % ('', 'f+d+w', total['ours'][0], total['ours'][1], total['a'][0], total['a'][1]), flush=True)


def bench_model(bs, route, sz=299):
    from neuralnetworklibrary_amd.Applications import Vision as V
    from neuralnetworklibrary_amd.Applications.VisionModels import inceptionresnetv2 as irn, vmods
    from neuralnetworklibrary_amd.General.Learner import Learner
    Learner.verbose = False
    if route == 'a':
        def forward(self, x):
            return route_a(self.conv2d, [getattr(self, 'branch%d' % i)(x) for i in range(self.n_branches)], x, self.scale, not self.noReLU)
        irn._Residual.forward = forward
    x, y = torch.randn(bs, 3, sz, sz, device='cuda'), torch.randint(0, 120, (bs,), device='cuda')
    data = types.SimpleNamespace(sz=(sz, sz), categories={i: str(i) for i in range(120)}, bs=bs, target_type='single_label')
    data.train_dl = [(None, torch.zeros(bs))]
    data.val_dl = data.train_dl
    torch.manual_seed(0)
    if route == 'fused':
        irn.Block17.fused = irn.Block8.fused = True                          # every class on the fused op, whatever the model ships with
    net = vmods.inceptionresnetv2()
    for m in net.modules():
        if route == 'a' and isinstance(m, irn._Residual) and 'nnl_hip_conv' in vars(m.conv2d):
            del m.conv2d.nnl_hip_conv                                         # route (a) runs it: back into the prepared-filter window
    model = V.ImageClassificationNet(data, net).cuda()
    learner = Learner('/tmp/nnl_bench_catproj', data, model, optimizer='SGD_Mom')
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
    print('inceptionresnetv2 train1minibatch bs %d at %d, residual tails on %s: median %.1f ms (min %.1f, max %.1f) over %d steps after 2 '
          'warm-up steps (loss %.4f)' % (bs, sz, {'fused': 'the fused op', 'a': 'route (a)', 'model': "the model's own routes"}[route], statistics.median(steady), min(steady),
                                         max(steady), len(steady), loss), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--model-bs', type=int, default=32)
    ap.add_argument('--skip-shapes', action='store_true')
    ap.add_argument('--route', choices=('fused', 'a', 'model'), default=None, help='time the whole step on this route only (no second process)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_catproj.py measures on the GPU: none is visible')
    if a.route is None and not a.skip_shapes:
        bench_shapes(a.bs, a.iters)
    if a.model_bs:
        bench_model(a.model_bs, a.route or 'fused')
        for route in ('a', 'model') if a.route is None else ():              # each in a process of its own
            subprocess.run([sys.executable, os.path.abspath(__file__), '--model-bs', str(a.model_bs), '--route', route], check=True)
