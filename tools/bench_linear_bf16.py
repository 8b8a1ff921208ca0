"""bf16 matrix-core Linear (csrc/linear_bf16.hip, ops.linear_bf16) against today's fp32 route (ops.linear: the fp32-MFMA implicit-GEMM
kernels on a 1x1 image) at the language model's large GEMMs: the tied decoder (M 4480 = 64 x 70, K 400, N 47 343) and the input
projections gx of the three LSTM layers (K 400 / 1150 / 1150 -> N 4600 / 4600 / 1600), forward, dgrad and wgrad.

Per direction: time per launch by HIP events through the autograd ops of both routes (forward: the op under no_grad; dgrad / wgrad:
torch.autograd.grad of a kept graph in which x / the weight alone requires a gradient; dy arrives as the view over a registered zero-padded base that
_SoftmaxCE and the LSTM backward hand over) — after a warm-up, three alternations of (bf16, fp32), each a block of `--iters` launches; the
median of the three blocks with min - max — against the bound max(flop over the 2516.6 TFLOP/s bf16 peak, the three fp32 tensors of the
call read or written once over 6.29 TB/s).  Before a shape is timed, the two routes' outputs are compared at the timed size.
Then Learner.train1minibatch of the AWD-LSTM language model (400 / 1150 / 3, V = 47 343, bs 64 x bptt 70) with use_bf16_linear() off
and on, alternated three times.
Every GPU step (a shape, the model) runs in a child process of its own under `timeout`; the tool stops at the first failure.
Usage: python tools/bench_linear_bf16.py [--iters 10] [--skip-shapes] [--skip-model] [--step-timeout 240]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS, BF16_TFLOPS = 6.29, 2516.6
V, BS, BPTT = 47343, 64, 70
SHAPES = [('decoder', BS * BPTT, 400, V), ('gx layer 1', BS * BPTT, 400, 4600), ('gx layer 2', BS * BPTT, 1150, 4600), ('gx layer 3', BS * BPTT, 1150, 1600)]


def block_us(fn, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def alternate(ours, base, iters):
    "((median, min, max) of ours, of the baseline) in us over three alternations after a warm-up"
    import torch
    for fn in (ours, base):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(3):
        a.append(block_us(ours, iters))
        b.append(block_us(base, iters))
    return (statistics.median(a), min(a), max(a)), (statistics.median(b), min(b), max(b))


def bench_shape(i, iters):
    import torch

    from neuralnetworklibrary_amd import ops
    name, M, K, N = SHAPES[i]
    dev = 'cuda'
    torch.manual_seed(i)
    x, w = torch.randn(M, K, device=dev, requires_grad=True), (torch.randn(N, K, device=dev) / K ** 0.5).requires_grad_(True)
    ld = (N + 15) // 16 * 16
    base = torch.zeros(M, ld, device=dev)
    base[:, :N] = torch.randn(M, N, device=dev)
    ops.register_padded_grad(base, ld)
    dy = base[:, :N] if ld != N else base
    flop = 2.0 * M * N * K
    bound = max(flop / (BF16_TFLOPS * 1e6), 4.0 * (M * K + N * K + M * N) / (HBM_TBS * 1e6))
    routes = {'bf16': ops.linear_bf16, 'fp32': ops.linear}
    # one kept graph per route and direction, with only that direction's input requiring a gradient
    ys = {(k, kind): f(x if kind == 'dgrad' else x.detach(), w if kind == 'wgrad' else w.detach()) for k, f in routes.items() for kind in ('dgrad', 'wgrad')}

    def call(route, kind):
        if kind == 'fwd':
            with torch.no_grad():
                return routes[route](x, w)
        return torch.autograd.grad(ys[route, kind], x if kind == 'dgrad' else w, dy, retain_graph=True)[0]
    for kind in ('fwd', 'dgrad', 'wgrad'):
        o16, o32 = call('bf16', kind), call('fp32', kind)
        rel = ((o16 - o32).abs().max() / o32.abs().max()).item()
        assert rel < 0.05, '%s %s: the two routes differ by %.3f of the largest value' % (name, kind, rel)
        del o16, o32
        (t, lo, hi), (tb, lob, hib) = alternate(lambda: call('bf16', kind), lambda: call('fp32', kind), iters)
        print('%-26s %-5s | %8.1f %8.1f-%8.1f | %8.1f %8.1f-%8.1f | %7.2f | %8.1f %7.2f' % (
            '%s %dx%d>%d' % (name, M, K, N), kind, t, lo, hi, tb, lob, hib, tb / t, bound, t / bound), flush=True)


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
    learner = Learner('/tmp/nnl_bench_linear_bf16', data, LanguageModelNet(_Vocab(stoi, BS)), optimizer='Adam', loss_func=RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(wd=1e-6, clip=0.4)

    def steps(flag, n):
        learner.use_bf16_linear(flag)
        ts, loss = [], None
        for j in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = learner.train1minibatch(*batches[j % 4], [1e-3, 1e-3], betas_batch=(0.8, 0.99))
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts[2:], loss                                               # two warm-up steps after every switch
    res, last = {True: [], False: []}, {}
    for _ in range(3):
        for flag in (True, False):
            ts, last[flag] = steps(flag, 8)
            res[flag].append(statistics.median(ts))
    for flag in (False, True):
        print('LM train1minibatch 400/1150/3 V %d bs %d x bptt %d, %s Linear: median %.2f ms (min %.2f - max %.2f over three alternations of 6 steps), last loss %.4f'
              % (V, BS, BPTT, 'bf16' if flag else 'fp32', statistics.median(res[flag]), min(res[flag]), max(res[flag]), last[flag]), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--skip-shapes', action='store_true')
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--child', default=None, help='internal: one GPU step, `shape:<index>` or `model`')
    a = ap.parse_args()
    if a.child:
        bench_model() if a.child == 'model' else bench_shape(int(a.child.split(':')[1]), a.iters)
        sys.exit(0)
    jobs = ([] if a.skip_shapes else ['shape:%d' % i for i in range(len(SHAPES))]) + ([] if a.skip_model else ['model'])
    if not a.skip_shapes:
        print('%-26s %-5s | %8s %17s | %8s %17s | %7s | %8s %7s' % ('shape M x K > N', 'dir', 'bf16 us', 'min - max', 'fp32 us', 'min - max', 'fp32/bf', 'bound us', 'x bound'),
              flush=True)
    for job in jobs:                                                      # each GPU step under its own time limit; the first failure ends the run
        rc = subprocess.run(['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--child', job, '--iters', str(a.iters)]).returncode
        if rc != 0:
            sys.exit('bench_linear_bf16: step %s ended with status %d: stopping' % (job, rc))
