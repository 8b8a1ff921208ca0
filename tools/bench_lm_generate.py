"""Text generation on the GPU: LanguageModelNet.predict_from_tokens(refeed=False) — the prompt through the encoder once, then per token three
nnl_lstm_cell_b1 launches and the two of nnl_lm_next_token, nothing read back until all n steps are enqueued — against the same decoder
written from what the tree had before those kernels: per token the existing encoder at T = 1 (ops.lstm_layer: MFMA GEMM with one live
row + the recurrence kernels), ops.linear for the tied decoder, F.softmax, torch.topk, and the seeded draw on the host after a read-back.
Full-size model (400 / 1150 / 3, V = 47 343), a prompt of `--prompt` tokens, `--n` new ones.

Before anything is timed both paths run on the golden G20's net (V = 61, logits spread over a few units) with a seed at which the fp64
restatement of tests/test_lm_generate.py has margins above 100 x its own fp32-fp64 distance: there both must give the restatement's
tokens (asserted).  At full size the freshly initialised model is nearly uniform and no margin can be asserted: the tool reports whether
the two token sequences agree and, if not, where they part.  One warm-up of each, then `--rounds` alternations; medians and spread.
`us_per_token` is the whole call divided by n (prompt pass, padded weight copies, upload and copy back included); `marginal` is the
difference to a call with n / 4 tokens divided by the extra tokens, against the traffic floor (every LSTM weight and the embedding
read once per token at 6.29 TB/s); `host_enqueue_marginal` is the same difference of the host time the n steps take to enqueue (they
return before the device has run them): under `marginal`, the loop is device-bound.
Usage: python tools/bench_lm_generate.py [--n 200] [--prompt 20] [--rounds 3] [--k 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_lm_generate as R  # noqa: E402  (the fp64 restatement and its margins)
from neuralnetworklibrary_amd import ops  # noqa: E402
from neuralnetworklibrary_amd.Applications.Text import LanguageModelNet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=200)
ap.add_argument('--prompt', type=int, default=20)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--k', type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
DEV = 'cuda'
COPY_RATE = 6.29e12


def baseline(net, ids, n, k=5, seed=0):
    "refeed=False's semantics on the existing encoder, ops.linear, torch's softmax / topk and a host draw: one read-back per token"
    u = R.uniforms(seed, n)
    emb = net.enc.word_embed.embed.weight
    net.eval()
    net.enc.reset(1)
    toks = list(ids)
    try:
        with torch.no_grad():
            x = torch.tensor([toks], device=emb.device)
            for i in range(n):
                enc_out = net.enc(x)
                p = F.softmax(ops.linear(enc_out[-1], emb)[0], dim=0)
                p[:net.N_SPECIAL] = 0
                tp, ti = torch.topk(p, k)
                cs = np.zeros(k, dtype=np.float32)
                c = np.float32(0)
                for m, v in enumerate(tp.cpu().numpy()):
                    c = np.float32(c + v)
                    cs[m] = c
                j = int((cs[:-1] <= np.float32(u[i] * cs[-1])).sum())
                toks.append(int(ti[j].item()))
                x = torch.tensor([[toks[-1]]], device=emb.device)
    finally:
        net.enc.reset(net.bs)
    return toks


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


# ---- agreement at a shape with asserted margins --------------------------------------------------------------------------------
g = R.load_golden('g20_lm_generate')
small = R.product_net(int(g['V']), int(g['tag']), float(g['scale']), DEV)
prompt_s = [int(t) for t in g['prompt']]
seed, want, _, _, d = R.seeds_with_margin(R.lm_params(small), prompt_s, 8, a.k, refeed=False)[0]
got_k = small.predict_from_tokens(prompt_s, 8, k=a.k, seed=seed, refeed=False)
got_b = baseline(small, prompt_s, 8, a.k, seed)
assert got_k == want, 'kernels part from the fp64 restatement: %r vs %r' % (got_k, want)
assert got_b == want, 'baseline parts from the fp64 restatement: %r vs %r' % (got_b, want)
del small

# ---- full size ---------------------------------------------------------------------------------------------------------------------
V = 47343
torch.manual_seed(0)
net = LanguageModelNet(R.vocab(V)).to(DEV)
prompt = [int(t) for t in np.random.RandomState(1).randint(4, V, a.prompt)]
enqueue_ms = []                                   # host time of the n steps alone: they return before the device has run them
_steps = net._generate_steps


def _timed_steps(*args, **kw):
    t = time.perf_counter()
    _steps(*args, **kw)
    enqueue_ms.append((time.perf_counter() - t) * 1e3)


net._generate_steps = _timed_steps
n_short = max(a.n // 4, 1)
ours = lambda n: (lambda: net.predict_from_tokens(prompt, n, k=a.k, seed=0, refeed=False))
base = lambda n: (lambda: baseline(net, prompt, n, a.k, 0))
_, tk = timed(ours(a.n))
_, tb = timed(base(a.n))
timed(ours(n_short)); timed(base(n_short))
parts = next((i for i, (x, y) in enumerate(zip(tk, tb)) if x != y), None)
res = {'kernels': {a.n: [], n_short: []}, 'baseline': {a.n: [], n_short: []}}
enq = {a.n: [], n_short: []}
for _ in range(a.rounds):
    for n in (a.n, n_short):
        res['baseline'][n].append(timed(base(n))[0])
        res['kernels'][n].append(timed(ours(n))[0])
        enq[n].append(enqueue_ms[-1])
sizes = [400, 1150, 1150, 400]
bytes_per_token = 4.0 * (sum(4 * sizes[i + 1] * (R._ceil4(sizes[i]) + R._ceil4(sizes[i + 1])) for i in range(3)) + V * 400)
floor_us = bytes_per_token / COPY_RATE * 1e6
out = {'V': V, 'prompt': a.prompt, 'n': a.n, 'k': a.k, 'rounds': a.rounds, 'bytes_per_token_MB': bytes_per_token / 1e6, 'floor_us': floor_us,
       'small_shape_tokens_equal_restatement': True, 'small_shape_seed': seed,
       'full_size_tokens_equal': parts is None, 'full_size_part_at_new_token': None if parts is None else parts - len(prompt)}
for name, r in res.items():
    per_tok = [t * 1e3 / a.n for t in r[a.n]]
    marg = [(tl - ts) * 1e3 / (a.n - n_short) for tl, ts in zip(r[a.n], r[n_short])] if a.n > n_short else []
    out[name] = {'call_ms': {'median': float(np.median(r[a.n])), 'spread': max(r[a.n]) - min(r[a.n]), 'all': r[a.n]},
                 'us_per_token': {'median': float(np.median(per_tok)), 'spread': max(per_tok) - min(per_tok)},
                 'marginal_us_per_token': {'median': float(np.median(marg)), 'spread': max(marg) - min(marg)} if marg else None}
if out['kernels']['marginal_us_per_token']:
    host = [(el - es) * 1e3 / (a.n - n_short) for el, es in zip(enq[a.n], enq[n_short])]
    out['kernels']['host_enqueue_marginal_us_per_token'] = {'median': float(np.median(host)), 'spread': max(host) - min(host)}
    out['kernels']['marginal_over_floor'] = out['kernels']['marginal_us_per_token']['median'] / floor_us
print(json.dumps(out))
