"""The text data side at an IMDB-like shape: `--texts` generated reviews (seeded generator below: Zipf-distributed words over a vocabulary of
`--words` strings, sentence punctuation, contractions, all-capitals words, numbers, <br /> breaks; about 1.3 kB per text — IMDB's train
split is 25 000 texts, about 33 MB) through TextDataset(strings, labels, tokenizer=Tokenizer()).  Nothing is read from disk.

Reported, as medians over `--rounds` alternations with the host baseline after one warm-up of everything, with the spread (min .. max):
  pre_ms      the host pre-rules (four re.sub per text) and the UTF-8 encoding
  upload_ms   the one upload of offsets + bytes                                          (host clock around a device synchronise)
  kernel_ms   the launches, HIP events on the stream around each phase (count, fill, hash + insert + verify, compact, assign + ids), summed,
              next to their traffic bound: every byte read once, every token record (8 B) written and read once, every id (8 B) written
              once, over the 6.29 TB/s copy rate
  back_ms     the copy back of ids + offsets, the per-text lists, the Series and the stoi dict
  total_ms    the public call, end to end
  host_ms     the baseline with the same results, checked before anything is timed: the same pre-rules, the grammar as ONE Python `re`
              pattern plus the case rule, collections.Counter, dict lookups
A row that cannot be measured is printed as "not measured".  No number gates anything.
Usage: python tools/bench_text_tokens.py [--texts 25000] [--words 80000] [--rounds 3] [--seed 0]"""
import argparse
import collections
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import ops_text as ot  # noqa: E402
from neuralnetworklibrary_amd.Applications.Text import TextDataset, Tokenizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--texts', type=int, default=25000)
ap.add_argument('--words', type=int, default=80000)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--seed', type=int, default=0)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
HBM = 6.29e12


def generate(n, n_words, seed):
    rs = np.random.RandomState(seed)
    letters = np.array(list('etaoinshrdlucmfwypvbgkqjxz'))
    vocab = [''.join(rs.choice(letters, rs.randint(2, 10))) for _ in range(n_words)]
    extra = ["don't", "it's", "couldn't", "I'm", "they're", 'GREAT', 'WORST', 'DVD', '10/10', '3.5', '1,000', 'café', '--', '<br /><br />']
    texts = []
    for _ in range(n):
        words = rs.zipf(1.25, rs.randint(60, 400))
        out = []
        for w in words:
            r = rs.random_sample()
            tok = extra[int(r * 1000) % len(extra)] if r < 0.04 else vocab[int(w - 1) % n_words]
            if r > 0.93:
                tok = tok.capitalize()
            out.append(tok + (rs.choice(['.', ',', '!', '?', '...', ' -']) if r > 0.85 else ''))
        texts.append(' '.join(out))
    return texts


RAW = rb'[0-9A-Za-z_\x80-\xff]'
WB = rb'(?:' + RAW + rb'|(?<=[0-9])[.,](?=[0-9]))'
SPECIAL = rb'<(?:eos|bos|unk)>'
NT = rb"[nN]'[tT](?!" + RAW + rb')'
WORD = rb'(?:(?!' + NT + rb')' + WB + rb')'
GRAMMAR = re.compile(rb'|'.join([SPECIAL, NT, rb'(?<=' + RAW + rb")'(?=" + RAW + rb')' + WORD + rb'*', WORD + rb'+',
                                 rb'(?!' + SPECIAL + rb')([^\s0-9A-Za-z_\x80-\xff])(?:(?!' + SPECIAL + rb')\1)*']))
RUN, UP, LOW = re.compile(RAW + rb'+'), re.compile(rb'[A-Z]'), re.compile(rb'[a-z]')


def host_tokens(b):
    out = []
    for m in GRAMMAR.finditer(b):
        s = m.start()
        run = RUN.match(b, s)
        if run and run.end() - s > 2 and (s == 0 or not RUN.match(b, s - 1)) and UP.search(run.group()) and not LOW.search(run.group()):
            out.append(b't_up')
        out.append(m.group().lower())
    return out


def host_baseline(texts, tok, max_vocab=60000, min_freq=6):
    ss = [host_tokens(tok.pre_rules(t).encode('utf-8')) for t in texts]
    common = collections.Counter(t for s in ss for t in s).most_common(max_vocab)
    names = [s.encode() for s in ot.TEXT_SPECIALS] + [t for t, c in common if c >= min_freq]
    stoi = {t: i for i, t in enumerate(names)}
    return [[stoi.get(t, 0) for t in s] for s in ss], {k.decode('utf-8'): v for k, v in stoi.items()}


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def phases(texts, tok):
    "TextDataset(texts, ..., tokenizer=tok)'s fused route phase by phase, through the same ops"
    pre, enc = clock(lambda: [tok.pre_rules(t).encode('utf-8', 'surrogateescape') for t in texts])
    up, corpus = clock(lambda: ot.TextCorpus.from_texts(enc))
    dev = corpus.bytes.device
    mode = ot.TEXT_MODE_GRAMMAR
    ntiles = (corpus.B + ot.TEXT_TILE - 1) // ot.TEXT_TILE
    tile_base = torch.empty(ntiles + 1, dtype=torch.int64, device=dev)
    k_count, _ = device_ms(lambda: ot.check(ot.lib.nnl_text_token_count(ot.ptr(corpus.bytes), corpus.B, ot.ptr(corpus.offsets), corpus.n, mode,
                                                                        ot.ptr(tile_base), ot.stream())))
    T = int(tile_base[-1].item())
    rec = torch.empty(2, T, dtype=torch.int32, device=dev)
    text_off = torch.empty(corpus.n + 1, dtype=torch.int64, device=dev)
    k_fill, _ = device_ms(lambda: ot.check(ot.lib.nnl_text_token_fill(ot.ptr(corpus.bytes), corpus.B, ot.ptr(corpus.offsets), corpus.n, mode,
                                                                      ot.ptr(tile_base), T, ot.ptr(rec[0]), ot.ptr(rec[1]), ot.ptr(text_off),
                                                                      ot.stream())))
    toks = ot.TextTokens(rec[0], rec[1], text_off, T, mode)
    table = ot.VocabTable(ot.vocab_capacity(T), dev)

    def build():
        keys = ot.token_hash(corpus, toks, ot.TEXT_SEEDS[0])
        slot = ot.vocab_insert(keys, T, table)
        return slot, ot.vocab_verify(corpus, toks, slot, table)
    k_build, (tok_slot, mism) = device_ms(build)
    assert int(mism.item()) == 0 and int(table.status.item()) == 0
    max_rows = min(table.cap, T)
    out = torch.zeros(max_rows * 5 + 1, dtype=torch.int32, device=dev)
    k_compact, _ = device_ms(lambda: ot.check(ot.lib.nnl_text_vocab_compact(ot.ptr(table.key), ot.ptr(table.count), ot.ptr(table.first), table.cap,
                                                                            ot.ptr(rec[0]), ot.ptr(rec[1]), T, ot.ptr(out), max_rows,
                                                                            ot.ptr(out[max_rows * 5:]), ot.stream())))
    K = int(out[-1].item())
    slots = out[:K * 5].view(K, 5)[:, 0].contiguous()
    slot_id = torch.empty(table.cap, dtype=torch.int32, device=dev)
    ids = torch.empty(T, dtype=torch.int64, device=dev)

    def finish():
        ot.check(ot.lib.nnl_text_vocab_assign(ot.ptr(slots), ot.ptr(slots), K, ot.ptr(slot_id), table.cap, ot.stream()))      # any ids: timing only
        ot.ids_write(tok_slot, slot_id, table.cap, toks, corpus.n, out=ids)
    k_ids, _ = device_ms(finish)
    return {'pre_ms': pre, 'upload_ms': up, 'kernel_ms': k_count + k_fill + k_build + k_compact + k_ids,
            'kernel_parts_ms': [k_count, k_fill, k_build, k_compact, k_ids], 'bytes': corpus.B, 'tokens': T, 'distinct': K,
            'bound_ms': (corpus.B + 24.0 * T) / HBM * 1e3}


def back_ms(texts, tok):
    "the public call minus everything before the copy back, measured as: the copy of ids + offsets, lists, Series, dict"
    import pandas as pd
    corpus = tok.corpus(texts)
    toks = ot.token_bounds(corpus, ot.TEXT_MODE_GRAMMAR)
    both = torch.zeros(toks.T + corpus.n + 1, dtype=torch.int64, device=corpus.bytes.device)
    both[toks.T:] = toks.text_off

    def back():
        host = both.cpu().numpy()
        res = ot.TextIds(host[:toks.T], host[toks.T:], None, None)
        return pd.Series(res.lists(), dtype=object), {str(i): i for i in range(60004)}
    return clock(back)[0]


def med(v):
    return '%.1f (%.1f .. %.1f)' % (statistics.median(v), min(v), max(v)) if v else 'not measured'


texts = generate(a.texts, a.words, a.seed)
labels = [i % 2 for i in range(len(texts))]
tok = Tokenizer()
ds = TextDataset(texts, labels, tokenizer=tok)                                   # warm-up of everything, and the check of the baseline
want_ids, want_stoi = host_baseline(texts, tok)
assert list(ds.texts) == want_ids and list(ds.stoi.items()) == list(want_stoi.items()), 'the host baseline and the device route disagree'
rows = collections.defaultdict(list)
info = {}
for _ in range(a.rounds):
    p = phases(texts, tok)
    for k in ('pre_ms', 'upload_ms', 'kernel_ms'):
        rows[k].append(p[k])
    info = p
    rows['back_ms'].append(back_ms(texts, tok))
    rows['total_ms'].append(clock(lambda: TextDataset(texts, labels, tokenizer=tok))[0])
    rows['host_ms'].append(clock(lambda: host_baseline(texts, tok))[0])
print('texts %d, bytes %d, tokens %d, distinct %d, vocabulary %d' % (len(texts), info['bytes'], info['tokens'], info['distinct'], len(ds.stoi)))
for k in ('pre_ms', 'upload_ms', 'kernel_ms', 'back_ms', 'total_ms', 'host_ms'):
    print('%-10s %s' % (k, med(rows[k])))
print('kernel parts (count, fill, hash+insert+verify, compact, assign+ids) ms: %s; traffic bound %.4f ms'
      % (', '.join('%.3f' % v for v in info['kernel_parts_ms']), info['bound_ms']))
print(json.dumps({'texts': len(texts), 'bytes': info['bytes'], 'tokens': info['tokens'], 'distinct': info['distinct'],
                  **{k: statistics.median(v) for k, v in rows.items()}, 'bound_ms': info['bound_ms']}))
