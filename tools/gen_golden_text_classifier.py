"""Golden vectors G17 for the text classifier (reference Applications/Text.py:127-180, 334-440, 575-609, 704-751).

Runs the REAL reference on CPU through oracle/_ref_import.py (read-only; oracle/synth.py for closed-form parameters) and writes
data only to tests/golden/g17_text_classifier.npz:
  (a) TextClassificationDecoder(emb 16, classes 3, attn 12, fc [10], drops 0), fill_module_ init, ragged pad-1 rows: pred, attn,
      every parameter gradient and d enc_out for a loss that also weights attn;
  (b) TextLengthSampler (random=False; random=True under np.random.seed), TextLengthCollater, TextClassificationDataObj batches;
  (c) the full-size TextClassificationNet (400 / 1150 / 3, V = 60, dropout 0) from a LanguageModelNet with fill_lm_reference_init_:
      one RegSeqCrossEntropyLoss(2, 1) forward / backward and two Learner.train1minibatch steps (Adam betas (0.7, 0.99),
      lr [2e-4, 1e-3, 5e-3], clip 1.0);
  (d) a 10-step loss curve on length-bucketed batches (T 12 .. 120, the last batch ragged, bs 16, V = 500, lr [5e-5, 1e-4, 3e-4])
      at fp32 and fp64; the generator asserts that the reference's own fp32 and fp64 curves agree (as oracle/gen_golden_curves.py does for G14).
Usage: python tools/gen_golden_text_classifier.py   (needs the reference checkout the oracle shim points at)"""
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _ref_import, synth  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g17_text_classifier.npz')
SEP_LIMIT = 3e-4
R = _ref_import.load()
TX = R['Applications.Text']
Learner = R['General.Learner'].Learner
Optimizer = R['General.Optimizer'].Optimizer


def A(t):
    return t.detach().cpu().numpy().copy()


def ragged_tokens(B, T, lengths, V, tag, lo=2):
    "x [B, T] int64: row b holds lengths[b] tokens in [lo, V) followed by pad 1"
    rs = np.random.RandomState(tag)
    x = np.ones((B, T), dtype=np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rs.randint(lo, V, n)
    return x


def ref_dataset(texts, labels):
    "a reference TextDataset without its spaCy tokeniser: the attributes its __init__ would set from numericalised texts"
    import pandas as pd
    ds = TX.TextDataset.__new__(TX.TextDataset)
    ds.texts = pd.Series([list(map(int, t)) for t in texts])
    ds.num_tokens = sum(len(t) for t in ds.texts)
    ds.label_dict = {lab: i for i, lab in enumerate(sorted(set(labels)))}
    ds.labels = pd.Series([ds.label_dict[lab] for lab in labels])
    ds.stoi = {'_pad_': 1}
    return ds


def part_a(out):
    T, B, E = 9, 5, 16
    dec = TX.TextClassificationDecoder(E, 3, 12, [10], [0., 0.])
    synth.fill_module_(dec, seed=17)
    dec.train()
    x = torch.from_numpy(ragged_tokens(B, T, [9, 7, 4, 9, 2], 20, 1701))
    enc = synth.synth_input((T, B, E), 1702).requires_grad_(True)
    pred, attn = dec(x, enc)
    loss = (pred * synth.synth_input((B, 3), 1703)).sum() + (attn * synth.synth_input((T, B), 1704)).sum()
    loss.backward()
    out.update({'a.x': A(x), 'a.enc': A(enc), 'a.pred': A(pred), 'a.attn': A(attn), 'a.d_enc': A(enc.grad)})
    out['a.param_names'] = np.array([n for n, _ in dec.named_parameters()])
    for n, p in dec.named_parameters():
        out['a.grad.' + n] = A(p.grad)


def part_b(out):
    rs = np.random.RandomState(1711)
    N, bs, bpg = 37, 4, 2
    lengths = rs.randint(1, 25, N)
    texts = [list(rs.randint(4, 50, n)) for n in lengths]
    labels = list(rs.choice(['neg', 'pos', 'mid'], N))
    out['b.lengths'], out['b.tokens'], out['b.labels'] = lengths.astype(np.int64), np.concatenate(texts).astype(np.int64), np.array(labels)
    out['b.bs'], out['b.bpg'] = bs, bpg
    for tag, random in (('fixed', False), ('random', True)):
        ds = ref_dataset(texts, labels)
        np.random.seed(1712)
        s = TX.TextLengthSampler(ds, bs, bpg, random=random)
        batches = [list(b) for b in s]
        out['b.%s.perm' % tag] = np.array(ds.perm, dtype=np.int64)
        out['b.%s.len' % tag] = np.array(len(s), dtype=np.int64)
        out['b.%s.batches' % tag] = np.concatenate(batches).astype(np.int64)
        out['b.%s.batch_sizes' % tag] = np.array([len(b) for b in batches], dtype=np.int64)
        out['b.%s.sorted_labels' % tag] = np.array(list(ds.labels), dtype=np.int64)
    ds = ref_dataset(texts, labels)
    TX.TextLengthSampler(ds, bs, bpg)
    xb, yb = TX.TextLengthCollater(1)([ds[i] for i in (5, 6, 7)])
    out['b.collate.x'], out['b.collate.y'] = A(xb), A(yb)
    # the data object: one epoch of its shuffled train loader and its val loader
    tr, va = ref_dataset(texts, labels), ref_dataset(texts[:11], labels[:11])
    np.random.seed(1713)
    d = TX.TextClassificationDataObj(tr, va, None, bs, bpg, num_workers=0)
    assert d.target_type == 'text_classify'
    xs = [(A(x), A(y)) for x, y in d.train_dl]
    out['b.obj.train_x'] = np.concatenate([x.reshape(-1) for x, _ in xs])
    out['b.obj.train_shapes'] = np.array([x.shape for x, _ in xs], dtype=np.int64)
    out['b.obj.train_y'] = np.concatenate([y for _, y in xs])
    out['b.obj.val_y'] = np.concatenate([A(y) for _, y in d.val_dl])


class _D:
    pass


def classifier(V, bs, dtype=torch.float32, path='/tmp/nnl_golden_g17'):
    d = _D()
    d.stoi = {('tok%d' % i): i for i in range(V)}
    d.stoi['_pad_'] = 1
    del d.stoi['tok1']
    d.bs, d.target_type = bs, 'text_classify'
    lm = TX.LanguageModelNet(d, enc_drops=[0., 0., 0., 0.], dec_drop=0.)
    lm.clear_non_raw()
    synth.fill_lm_reference_init_(lm, seed=17)
    net = TX.TextClassificationNet(path, lm, 3, enc_drops=[0., 0., 0., 0.], fc_drops=[0., 0.])
    net.clear_non_raw()
    synth.fill_module_(net.dec, seed=18)
    return net.to(dtype).train(), d


def part_c(out):
    V, bs, T = 60, 4, 7
    net, d = classifier(V, bs)
    x = torch.from_numpy(ragged_tokens(bs, T, [7, 5, 7, 3], V, 1721, lo=4))
    y = torch.from_numpy(np.random.RandomState(1722).randint(0, 3, bs).astype(np.int64))
    x2 = torch.from_numpy(ragged_tokens(bs, T - 2, [5, 5, 4, 2], V, 1723, lo=4))
    y2 = torch.from_numpy(np.random.RandomState(1724).randint(0, 3, bs).astype(np.int64))
    out.update({'c.x0': A(x), 'c.y0': A(y), 'c.x1': A(x2), 'c.y1': A(y2)})
    lf = TX.RegSeqCrossEntropyLoss(2.0, 1.0)
    outp = net(x)
    loss = lf(outp, y)
    loss.backward()
    out['c.loss'], out['c.ce'], out['c.pred'] = A(loss), A(lf.cross_entropy), A(outp[0])
    out['c.param_names'] = np.array([n for n, _ in net.named_parameters()])
    out['c.grad_norms'] = np.array([p.grad.norm().item() for _, p in net.named_parameters()], dtype=np.float64)
    sd = dict(net.named_parameters())
    out['c.grad.attn1_slice'] = A(sd['dec.attn1.weight'].grad)[:16, :64].copy()
    out['c.grad.attn2'] = A(sd['dec.attn2.weight'].grad)
    out['c.grad.emb'] = A(sd['enc.word_embed.embed.weight'].grad)
    out['c.grad.whh2_slice'] = A(sd['enc.lstms.2.lstm.weight_hh_l0_raw'].grad)[:64, :64].copy()
    net, d = classifier(V, bs)
    batches = [(x, y), (x2, y2)]
    d.train_dl, d.val_dl = batches, batches
    opt = Optimizer(partial(torch.optim.Adam, betas=(0.7, 0.99)), net)
    learner = Learner('/tmp/nnl_golden_g17', d, net, opt, TX.RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(clip=1.0)
    net.train()
    out['c.step_losses'] = np.array([learner.train1minibatch(xb, yb, [2e-4, 1e-3, 5e-3], betas_batch=(0.7, 0.99)) for xb, yb in batches],
                                    dtype=np.float64)
    out['c.after.abs_sums'] = np.array([p.double().abs().sum().item() for _, p in net.named_parameters()], dtype=np.float64)


def curve_batches(V=500, bs=16, steps=10):
    "length-bucketed, end-padded batches: T_i from 12 to 120, labels = whether marker token 7 occurs; the last batch has 9 rows"
    rs = np.random.RandomState(1731)
    Ts = rs.permutation(np.linspace(12, 120, steps).astype(np.int64))
    out = []
    for i, T in enumerate(Ts):
        n = bs if i < steps - 1 else 9
        lengths = np.maximum(T - rs.randint(0, 8, n), 2)
        lengths[0] = T
        x = np.ones((n, T), dtype=np.int64)
        y = rs.randint(0, 2, n).astype(np.int64)
        for b in range(n):
            x[b, :lengths[b]] = rs.randint(8, V, lengths[b])
            if y[b]:
                x[b, rs.randint(0, lengths[b])] = 7
        out.append((x, y))
    return out


def part_d(out):
    V, bs, steps = 500, 16, 10
    lr = [5e-5, 1e-4, 3e-4]        # Adam's first updates are ~lr * sign(g): at larger rates the reference's own fp32 / fp64 runs part
    batches = curve_batches(V, bs, steps)
    for i, (x, y) in enumerate(batches):
        out['d.x%d' % i], out['d.y%d' % i] = x.astype(np.int16), y
    out['d.steps'], out['d.V'], out['d.bs'], out['d.lr'] = steps, V, bs, np.array(lr)
    for tag, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        torch.set_default_dtype(dtype)                     # the encoder's per-forward zero state (Text.py:531-533) follows it
        try:
            net, d = classifier(V, bs, dtype)
            d.train_dl = d.val_dl = [(None, torch.zeros(bs))]
            opt = Optimizer(partial(torch.optim.Adam, betas=(0.7, 0.99)), net)
            learner = Learner('/tmp/nnl_golden_g17', d, net, opt, TX.RegSeqCrossEntropyLoss(2.0, 1.0))
            learner.init_optimizer(clip=1.0)
            net.train()
            losses = []
            for i, (x, y) in enumerate(batches):
                losses.append(learner.train1minibatch(torch.from_numpy(x), torch.from_numpy(y), lr, betas_batch=(0.7, 0.99)))
                print(tag, i, x.shape, losses[-1], flush=True)
        finally:
            torch.set_default_dtype(torch.float32)
        out['d.losses.' + tag] = np.array(losses, dtype=np.float64)
        out['d.after.abs_sums.' + tag] = np.array([p.double().abs().sum().item() for _, p in net.named_parameters()], dtype=np.float64)
    sep = np.abs(out['d.losses.f32'] - out['d.losses.f64']) / np.abs(out['d.losses.f64'])
    print('g17(d) fp32-vs-fp64 relative separation per step:', np.array2string(sep, precision=1), flush=True)
    assert sep.max() < SEP_LIMIT, 'g17(d): the reference itself separates by %.1e: fixture not well conditioned' % sep.max()


def main():
    out = {}
    for part in (part_a, part_b, part_c, part_d):
        part(out)
        print(part.__name__, 'done', flush=True)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, '%.1f KB' % (os.path.getsize(OUT) / 1024))


if __name__ == '__main__':
    main()
