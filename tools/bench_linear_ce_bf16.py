"""Fused bf16 decoder + softmax cross-entropy (csrc/linear_ce_bf16.hip, ops.linear_cross_entropy_bf16) against the route it replaces,
ops.softmax_cross_entropy(ops.linear_bf16(x, w), target), at the language model's tied decoder: M 4480 = 64 x 70, K 400, N 47 343.

Forward: the loss under no_grad.  Backward: torch.autograd.grad of a kept graph for (dx, dw) — fused: the two recomputing kernels and the
dx fold; unfused: softmax_ce_bwd, dgrad and wgrad.  Time per call by HIP events: after a warm-up, three alternations of (fused, unfused),
each a block of `--iters` calls; the median of the three blocks with min - max.  torch.cuda.max_memory_allocated of one forward + backward
of each route, above what the operands hold.  Before anything is timed the two routes' losses and gradients are compared.
Then Learner.train1minibatch of the AWD-LSTM language model (400 / 1150 / 3, V = 47 343, bs 64 x bptt 70) under use_bf16_linear(), with
use_fused_decoder_loss() off and on, alternated three times, with the peak memory of a step of each.
Every GPU step runs in a child process of its own under `timeout`; the tool stops at the first failure.
Usage: python tools/bench_linear_ce_bf16.py [--iters 10] [--skip-op] [--skip-model] [--step-timeout 240]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_linear_bf16 import alternate  # noqa: E402

V, BS, BPTT, K = 47343, 64, 70, 400


def bench_op(iters):
    import torch

    from neuralnetworklibrary_amd import ops
    M, dev = BS * BPTT, 'cuda'
    torch.manual_seed(0)
    x, w = torch.randn(M, K, device=dev, requires_grad=True), (torch.randn(V, K, device=dev) / K ** 0.5).requires_grad_(True)
    t = torch.randint(0, V, (M,), device=dev)
    routes = {'fused': lambda: ops.linear_cross_entropy_bf16(x, w, t), 'unfused': lambda: ops.softmax_cross_entropy(ops.linear_bf16(x, w), t)}

    def fwd(route):
        with torch.no_grad():
            return routes[route]()
    peak, out = {}, {}
    for route, f in routes.items():                                     # one forward + backward: the comparison and the peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        loss = f()
        out[route] = (loss.detach(),) + torch.autograd.grad(loss, (x, w))
        torch.cuda.synchronize()
        peak[route] = torch.cuda.max_memory_allocated() - held
        del loss
    for a, b, what in zip(out['fused'], out['unfused'], ('loss', 'dx', 'dw')):
        rel = ((a - b).abs().max() / b.abs().max()).item()
        assert rel < 0.02, '%s: the two routes differ by %.4f of the largest value' % (what, rel)
    del out
    kept = {route: f() for route, f in routes.items()}                  # (the unfused graph keeps its logits, as a training step does)
    calls = {'fwd': fwd, 'bwd': lambda route: torch.autograd.grad(kept[route], (x, w), retain_graph=True)}
    print('decoder %d x %d > %d    |  fused us     min - max      | unfused us    min - max      | unfused/fused' % (M, K, V))
    for kind, call in calls.items():
        (tf, lo, hi), (tu, lou, hiu) = alternate(lambda: call('fused'), lambda: call('unfused'), iters)
        print('%-26s | %9.1f %8.1f-%8.1f | %9.1f %8.1f-%8.1f | %6.2f' % (kind, tf, lo, hi, tu, lou, hiu, tu / tf), flush=True)
    print('peak memory of one forward + backward above the operands: fused %.1f MB, unfused %.1f MB' % (peak['fused'] / 1e6, peak['unfused'] / 1e6), flush=True)


def bench_model():
    import types

    import torch

    from neuralnetworklibrary_amd.Applications.Text import LanguageModelNet, RegSeqCrossEntropyLoss, _Vocab
    from neuralnetworklibrary_amd.General.Core import set_default_device
    from neuralnetworklibrary_amd.General.Learner import Learner
    Learner.verbose = False
    set_default_device('cuda')
    torch.manual_seed(1237)
    stoi = {i: i for i in range(V)}
    stoi['_pad_'] = 1
    del stoi[1]
    stream_ = torch.randint(4, V, (BS, BPTT * 4 + 1), device='cuda')
    batches = [(stream_[:, i * BPTT:(i + 1) * BPTT].contiguous(), stream_[:, i * BPTT + 1:(i + 1) * BPTT + 1].contiguous()) for i in range(4)]
    data = types.SimpleNamespace(bs=BS, target_type='lang_model', stoi=stoi, train_dl=batches, val_dl=batches)
    learner = Learner('/tmp/nnl_bench_linear_ce_bf16', data, LanguageModelNet(_Vocab(stoi, BS)), optimizer='Adam', loss_func=RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(wd=1e-6, clip=0.4)
    learner.use_bf16_linear()

    def steps(flag, n):
        learner.use_fused_decoder_loss(flag)
        ts, loss, peak = [], None, 0
        for j in range(n):
            torch.cuda.synchronize()
            if j == 2:
                torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            loss = learner.train1minibatch(*batches[j % 4], [1e-3, 1e-3], betas_batch=(0.8, 0.99))
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            peak = torch.cuda.max_memory_allocated()
        return ts[2:], loss, peak                                         # two warm-up steps after every switch
    res, last, peak = {True: [], False: []}, {}, {}
    for _ in range(3):
        for flag in (True, False):
            ts, last[flag], peak[flag] = steps(flag, 8)
            res[flag].append(statistics.median(ts))
    for flag in (False, True):
        print('LM train1minibatch 400/1150/3 V %d bs %d x bptt %d, bf16 Linear, decoder loss %s: median %.2f ms (min %.2f - max %.2f over three alternations of 6 '
              'steps), peak memory %.0f MB, last loss %.4f' % (V, BS, BPTT, 'fused' if flag else 'unfused', statistics.median(res[flag]), min(res[flag]),
                                                                max(res[flag]), peak[flag] / 1e6, last[flag]), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--skip-op', action='store_true')
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--child', default=None, help='internal: one GPU step, `op` or `model`')
    a = ap.parse_args()
    if a.child:
        bench_model() if a.child == 'model' else bench_op(a.iters)
        sys.exit(0)
    for job in ([] if a.skip_op else ['op']) + ([] if a.skip_model else ['model']):       # each GPU step under its own time limit; the first failure ends the run
        rc = subprocess.run(['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--child', job, '--iters', str(a.iters)]).returncode
        if rc != 0:
            sys.exit('bench_linear_ce_bf16: step %s ended with status %d: stopping' % (job, rc))
