"""Text classifier benchmark: prints ONE JSON line.

* decoder: TextClassificationDecoder forward + backward (attn1 GEMM included) at T in {300, 1000}, B = 64, E = 400, A = 100 —
  the fused attention-pooling kernels (ops_text.attention_pool) against the ATen composition the decoder ran before them
  (kept below as the baseline), in the same process, alternating, timed with device events — eager, and replayed from a
  captured graph (device time alone);
* kernels: nnl_attn_pool_fwd / _bwd alone (device time: the launches replayed from a captured graph), bytes moved (forward T*B*(E+A)*4, backward T*B*(2E+2A)*4) over kernel time, as a
  share of the 6.29 TB/s copy rate;
* steps: Learner.train1minibatch ms / step of the full-size TextClassificationNet (400 / 1150 / 3, V = 47 343, bs 64) at
  T in {75, 300, 1000}, encoder frozen (learner.freeze()) and unfrozen.
Usage: python tools/bench_text_classifier.py [--reps N] [--steps K] [--no-steps]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neuralnetworklibrary_amd import ops, ops_text  # noqa: E402
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402

COPY_TBS = 6.29
DEV = 'cuda'


def aten_decoder_tail(dec, h, enc_in, enc_out):
    "the decoder after attn1 as it ran before the fused kernels (attn2 GEMM, softmax, mask, renormalise, weighted sum)"
    attn = ops.linear(h, dec.attn2.weight, dec.attn2.bias).squeeze()
    attn = F.softmax(attn, dim=0)
    attn = attn * (enc_in.transpose(1, 0) != 1).float()
    attn = attn / attn.sum(dim=0).unsqueeze(0)
    return dec.fc((attn.unsqueeze(2) * enc_out).sum(0)), attn


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def graph_timed(launch, n):
    """device time per launch: n launches captured back to back in one graph and replayed (a ctypes call costs the host more
    than one of these kernels runs, so timing eager launches would time the host)"""
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(n):
                launch()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    return timed(g.replay, 3) / n


def decoder_case(Tn, B, E, A, reps):
    from neuralnetworklibrary_amd.Applications.Text import TextClassificationDecoder
    torch.manual_seed(0)
    dec = TextClassificationDecoder(E, 2, A, [100], [0., 0.]).to(DEV).train()
    enc_out = torch.randn(Tn, B, E, device=DEV, requires_grad=True)
    x = torch.randint(4, 1000, (B, Tn), device=DEV)
    x[B // 2:, Tn * 3 // 4:] = 1
    dpred = torch.randn(B, 2, device=DEV)

    def fused():
        pred, _ = dec(x, enc_out)
        pred.backward(dpred)

    def aten():
        h = ops.linear(enc_out, dec.attn1.weight, dec.attn1.bias, relu=True)
        pred, _ = aten_decoder_tail(dec, h, x, enc_out)
        pred.backward(dpred)
    for f in (fused, aten):
        f(); f()
    tf, ta = [], []
    for _ in range(5):                                   # alternate the two, 5 rounds of `reps`
        tf.append(timed(fused, reps))
        ta.append(timed(aten, reps))
    # the same two, replayed from captured graphs: device time without the host's launch cost
    gf, ga = [], []
    for _ in range(5):
        gf.append(graph_timed(fused, reps))
        ga.append(graph_timed(aten, reps))
    # the two kernels alone
    h = torch.relu(torch.randn(Tn, B, A, device=DEV))
    w2, b2 = torch.randn(A, device=DEV), torch.randn(1, device=DEV)
    attn, pooled = torch.empty(Tn, B, device=DEV), torch.empty(B, E, device=DEV)
    dh, denc, dw2, db2 = torch.empty_like(h), torch.empty_like(enc_out), torch.empty_like(w2), torch.empty_like(b2)
    dpo = torch.randn(B, E, device=DEV)
    wsb = int(lib.nnl_attn_pool_workspace_bytes(Tn, B, E, A))
    ws = torch.empty(wsb // 4, device=DEV)
    cnt = ops._tile_counters(torch.device(DEV))
    eo = enc_out.detach()
    fwd = lambda: check(lib.nnl_attn_pool_fwd(ptr(h), ptr(w2), ptr(b2), ptr(eo), ptr(x), 1, ptr(attn), ptr(pooled), Tn, B, E, A,
                                              ptr(ws), wsb, ptr(cnt), cnt.numel(), stream()))
    bwd = lambda: check(lib.nnl_attn_pool_bwd(ptr(h), ptr(w2), ptr(eo), ptr(attn), ptr(dpo), None, ptr(dh), ptr(denc), ptr(dw2),
                                              ptr(db2), Tn, B, E, A, ptr(ws), wsb, ptr(cnt), cnt.numel(), stream()))
    fwd(); bwd()
    kf = min(graph_timed(fwd, reps * 4) for _ in range(3))
    kb = min(graph_timed(bwd, reps * 4) for _ in range(3))
    fb, bb = Tn * B * (E + A) * 4, Tn * B * (2 * E + 2 * A) * 4
    med = lambda v: sorted(v)[len(v) // 2]
    return {'T': Tn, 'B': B, 'E': E, 'A': A, 'fused_fwd_bwd_ms': round(med(tf), 4), 'aten_fwd_bwd_ms': round(med(ta), 4),
            'speedup': round(med(ta) / med(tf), 3),
            'fused_fwd_bwd_replayed_ms': round(med(gf), 4), 'aten_fwd_bwd_replayed_ms': round(med(ga), 4),
            'speedup_replayed': round(med(ga) / med(gf), 3),
            'kernel_fwd_us': round(kf * 1e3, 2), 'kernel_bwd_us': round(kb * 1e3, 2),
            'fwd_bytes': fb, 'bwd_bytes': bb,
            'fwd_TBps': round(fb / (kf * 1e-3) / 1e12, 3), 'bwd_TBps': round(bb / (kb * 1e-3) / 1e12, 3),
            'fwd_share_of_copy': round(fb / (kf * 1e-3) / 1e12 / COPY_TBS, 3),
            'bwd_share_of_copy': round(bb / (kb * 1e-3) / 1e12 / COPY_TBS, 3)}


def step_case(Tn, steps, frozen):
    from neuralnetworklibrary_amd.Applications.Text import (LanguageModelNet, RegSeqCrossEntropyLoss, TextClassificationNet, _Vocab)
    from neuralnetworklibrary_amd.General.Learner import Learner
    V, bs = 47343, 64
    stoi = {i: i for i in range(V)}
    stoi['_pad_'] = 1
    del stoi[1]
    torch.manual_seed(0)
    lm = LanguageModelNet(_Vocab(stoi, bs))
    net = TextClassificationNet('/tmp/nnl_bench_textclf', lm, 2)

    class D:
        target_type = 'text_classify'
    D.bs = bs
    D.train_dl = D.val_dl = [(None, torch.zeros(bs))]
    learner = Learner('/tmp/nnl_bench_textclf', D(), net, optimizer='Adam', loss_func=RegSeqCrossEntropyLoss(2.0, 1.0))
    if frozen:
        learner.freeze()
    learner.init_optimizer(clip=0.25)
    net.train()
    g = torch.Generator().manual_seed(Tn)
    x = torch.randint(4, V, (bs, Tn), generator=g)
    x[bs // 2:, Tn - Tn // 8:] = 1
    x, y = x.to(DEV), torch.randint(0, 2, (bs,), generator=g).to(DEV)
    lr = [1e-4, 1e-4, 1e-3]
    for _ in range(2):
        learner.train1minibatch(x, y, lr, betas_batch=(0.7, 0.99))
    torch.cuda.synchronize()
    ms = timed(lambda: learner.train1minibatch(x, y, lr, betas_batch=(0.7, 0.99)), steps)
    del learner, net, lm
    torch.cuda.empty_cache()
    return {'T': Tn, 'bs': bs, 'V': V, 'frozen': frozen, 'ms_per_step': round(ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--no-steps', action='store_true')
    a = ap.parse_args()
    res = {'metric': 'text_classifier', 'copy_TBps': COPY_TBS,
           'decoder': [decoder_case(Tn, 64, 400, 100, a.reps) for Tn in (300, 1000)]}
    if not a.no_steps:
        res['train_step'] = [step_case(Tn, a.steps, frozen) for Tn in (75, 300, 1000) for frozen in (True, False)]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
