"""Text data side (K17) on the GPU: the token kernels against the tests' restatement of the grammar over tile and text boundaries, the
vocabulary kernels against Counter / most_common, the collision and overflow paths, and the string / file routes of the datasets end
to end.  Every comparison is exact.  Shapes are the smallest at which each kernel can go wrong."""
import collections
import os
import random

import numpy as np
import pytest
import torch

import text_tokens_restatement as R

# ---- token bounds ---------------------------------------------------------------------------------------------------------------

CONSTRUCTS = [b'straddle', b"don't", b"DON'T", b'<unk>', b'3.5', b'1,000', b'!!!!', b"it's", b'NASA']


def _boundary_corpus(TB):
    """About 300 texts laid end to end with NO separator.  Returns (data, offsets)."""
    rng = random.Random(3)
    words = [b'the', b'movie', b"wasn't", b'GOOD', b'3.5', b'--', b'<eos>', b"it's", b'x', b'caf\xc3\xa9', b'...', b'ok!']
    texts = [b'x', b'', b'   ', b' \n\t ']                                     # one byte (the buffer's first byte is in a token), empty, blank
    texts.append(b' '.join(rng.choice(words) for _ in range(3 * TB // 4 + 40)))   # longer than 3 TB
    assert len(texts[-1]) > 3 * TB
    texts.append(b'a' * (TB + 37))                                               # single tokens longer than TB
    texts.append(b'see ' + b'B' * (TB + 5) + b"N'T now")                          # ... and the case rule's run longer than TB
    size = lambda: sum(len(t) for t in texts)

    def filler(n):
        "a text of exactly n bytes that ends in a space"
        out = b''
        while len(out) < n:
            out += rng.choice(words) + b' '
        return out[:max(n - 1, 0)] + b' ' * min(n, 1)

    for c in CONSTRUCTS:
        for k in range(1, len(c)):
            # (a) inside one text, bytes c[:k] before a tile boundary and c[k:] after it
            edge = (size() // TB + 2) * TB
            texts.append(filler(edge - k - size()) + c + b' tail')
            assert (sum(len(t) for t in texts[:-1]) + len(texts[-1]) - 5 - len(c) + k) % TB == 0
            # (b) a text boundary inside it: two texts, two (or more) tokens
            texts.append(b'left ' + c[:k])
            texts.append(c[k:] + b' right')
        # (c) a text boundary ON a tile boundary with the construct cut by both
        edge = (size() // TB + 2) * TB
        k = len(c) // 2
        texts.append(filler(edge - k - size()) + c[:k])
        assert size() % TB == 0
        texts.append(c[k:])
    while len(texts) < 300:                                                     # more texts than tiles
        texts.append(rng.choice([b'hi', b'', b'ok go', b"CAN'T", b'?', b'a b c']))
    texts.append(b'no trailing space at the end')                               # the buffer's last byte is in a token
    off = [0]
    for t in texts:
        off.append(off[-1] + len(t))
    assert len(texts) > off[-1] // TB + 1
    return b''.join(texts), off


def _restated_records(data, off, mode):
    rec, tok_off = [], [0]
    for j in range(len(off) - 1):
        rec += [(s + off[j], l) for s, l in R.records(data[off[j]:off[j + 1]], mode)]
        tok_off.append(len(rec))
    return rec, tok_off


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [R.GRAMMAR_MODE, R.SPLIT_MODE], ids=['grammar', 'split'])
def test_token_bounds_equal_the_restatement_over_tile_and_text_boundaries(mode):
    from neuralnetworklibrary_amd import ops_text
    data, off = _boundary_corpus(ops_text.TEXT_TILE)
    corpus = ops_text.TextCorpus(data, off)
    toks = ops_text.token_bounds(corpus, mode)
    want, want_off = _restated_records(data, off, mode)
    assert toks.T == len(want)
    got = list(zip(toks.start[:toks.T].tolist(), toks.len[:toks.T].tolist()))
    assert got == want
    assert toks.text_off.tolist() == want_off
    strings = ops_text.token_strings(corpus, toks)
    for j in (0, 4, 5, 6, 40, 41, 42, len(off) - 2):
        assert strings[j] == R.tokens(data[off[j]:off[j + 1]], mode)
    again = ops_text.token_bounds(corpus, mode)                                # the same bytes on a second call
    assert torch.equal(again.start, toks.start) and torch.equal(again.len, toks.len) and torch.equal(again.text_off, toks.text_off)


@pytest.mark.gpu
@pytest.mark.parametrize('texts', [[b'', b'  ', b'\n\t'], [b'', b'']], ids=['blank', 'no-bytes'])
def test_a_buffer_without_tokens(texts):
    from neuralnetworklibrary_amd import ops_text
    corpus = ops_text.TextCorpus.from_texts(texts)
    for mode in (R.GRAMMAR_MODE, R.SPLIT_MODE):
        toks = ops_text.token_bounds(corpus, mode)
        assert toks.T == 0 and toks.text_off.tolist() == [0] * (len(texts) + 1)
        out = ops_text.text_numericalize(corpus, mode)
        assert out.lists() == [[] for _ in texts] and list(out.stoi) == ['_unk_', '_pad_', '_bos_', '_eos_']


# ---- vocabulary -----------------------------------------------------------------------------------------------------------------

def _vocab_lists():
    "about 5 000 tokens over about 600 distinct strings, counts planted in ties, spread over 40 texts in a seeded order"
    rng = random.Random(11)
    names = ['w%d' % i for i in range(590)] + ['É', "n't", 'UP', 'up', '3.5', '<unk>', 't_up', '_pad_', 'a' * 300, '!']
    bag = []
    for i, name in enumerate(names):
        bag += [name] * (1 + (i % 7) * 2 + (30 if i % 50 == 0 else 0))          # ~85 names share every count
    rng.shuffle(bag)
    cuts = sorted(rng.sample(range(1, len(bag)), 39))
    return [bag[a:b] for a, b in zip([0] + cuts, cuts + [len(bag)])]


@pytest.mark.gpu
@pytest.mark.parametrize('max_vocab,min_freq', [(60000, 6), (100, 2), (400, 5)])
def test_vocabulary_equals_counter_most_common(max_vocab, min_freq):
    from neuralnetworklibrary_amd import ops_text
    from neuralnetworklibrary_amd.Applications.Text import _split_corpus, numericalize
    ss = _vocab_lists()
    assert 4500 <= sum(len(s) for s in ss) <= 6000 and len({t for s in ss for t in s}) == 600
    want_ids, want_stoi = R.numericalize(ss, max_vocab, min_freq)
    counter = collections.Counter(t for s in ss for t in s)
    if max_vocab == 100:                       # the cut bites first: tokens frequent enough are lost to it
        assert sum(1 for c in counter.values() if c >= min_freq) > max_vocab == len(want_stoi) - 4
    ids, stoi = numericalize(ss, max_vocab, min_freq)
    assert ids == want_ids and list(stoi.items()) == list(want_stoi.items())
    corpus = _split_corpus(ss)
    a = ops_text.text_numericalize(corpus, ops_text.TEXT_MODE_SPLIT, max_vocab, min_freq)
    b = ops_text.text_numericalize(corpus, ops_text.TEXT_MODE_SPLIT, max_vocab, min_freq)
    assert list(a.counts.items()) == [(t, c) for t, c in counter.most_common(max_vocab) if c >= min_freq]
    assert a.ids.tobytes() == b.ids.tobytes() and a.offsets.tobytes() == b.offsets.tobytes()
    assert list(a.stoi.items()) == list(b.stoi.items()) and list(a.counts.items()) == list(b.counts.items())
    toks = ops_text.token_bounds(corpus, ops_text.TEXT_MODE_SPLIT)
    rows = [ops_text.vocab_compact(ops_text.vocab_build_exact(corpus, toks)[0], toks)[:, 1:] for _ in range(2)]
    assert rows[0].tobytes() == rows[1].tobytes() and len(rows[0]) == 600          # count, first, start, len: the same bytes twice


@pytest.mark.gpu
def test_given_stoi_maps_unseen_tokens_to_zero_even_on_an_occupied_key():
    from neuralnetworklibrary_amd import ops_text
    from neuralnetworklibrary_amd.Applications.Text import _split_corpus, numericalize
    ss = _vocab_lists()
    _, stoi = R.numericalize(ss, 100, 2)
    other = [s[::-1] + ['never_seen', 'w5', 'W5'] for s in ss[:10]]
    want, _ = R.numericalize(other, stoi=stoi)
    got, got_stoi = numericalize(other, stoi=stoi)
    assert got == want and got_stoi is stoi and any(0 in s for s in got)
    # an unseen token whose masked key equals a vocabulary string's key: the byte comparison, not the key, decides
    mask = 0xFF
    cand = ['c%d' % i for i in range(400)]
    corpus = _split_corpus([cand])
    toks = ops_text.token_bounds(corpus, ops_text.TEXT_MODE_SPLIT)
    keys = ops_text.token_hash(corpus, toks, ops_text.TEXT_SEEDS[0], mask)[:toks.T].tolist()
    vocab, seen = [], set()
    for name, key in zip(cand, keys):
        if key not in seen and len(vocab) < 24:
            vocab.append(name)
            seen.add(key)
    vkeys = {keys[cand.index(v)] for v in vocab}
    ghosts = [name for name, key in zip(cand, keys) if name not in vocab and key in vkeys]
    assert len(vocab) == 24 and ghosts
    small = {v: 10 + i for i, v in enumerate(vocab)}
    data = [vocab + ghosts[:3] + vocab[::-1]]
    out = ops_text.text_numericalize(_split_corpus(data), ops_text.TEXT_MODE_SPLIT, stoi=small, hash_mask=mask)
    assert out.lists() == R.numericalize(data, stoi=small)[0] and out.lists()[0].count(0) == len(ghosts[:3])


# ---- collisions and overflow: bounded loops, detected, never merged -------------------------------------------------------------------

@pytest.mark.gpu
def test_forced_collisions_are_reported_retried_and_raised(monkeypatch):
    from neuralnetworklibrary_amd import ops_text
    from neuralnetworklibrary_amd.Applications.Text import _split_corpus, numericalize
    ss = [['t%d' % ((i * 7) % 100) for i in range(j, j + 60)] for j in range(0, 300, 60)]
    assert len({t for s in ss for t in s}) == 100
    corpus = _split_corpus(ss)
    toks = ops_text.token_bounds(corpus, ops_text.TEXT_MODE_SPLIT)
    for seed in ops_text.TEXT_SEEDS:
        _, _, mism = ops_text.vocab_build(corpus, toks, seed, hash_mask=0xF)
        assert mism > 0
    with pytest.raises(RuntimeError, match='collision'):
        ops_text.vocab_build_exact(corpus, toks, hash_mask=0xF)
    with pytest.raises(RuntimeError, match='collision'):
        ops_text.text_numericalize(corpus, ops_text.TEXT_MODE_SPLIT, hash_mask=0xF)
    monkeypatch.setattr(ops_text, 'TEXT_HASH_MASK', 0xF)
    with pytest.raises(RuntimeError, match='collision'):
        numericalize(ss, min_freq=1)
    monkeypatch.undo()
    ids, stoi = numericalize(ss, min_freq=1)
    want_ids, want_stoi = R.numericalize(ss, min_freq=1)
    assert ids == want_ids and list(stoi.items()) == list(want_stoi.items())


@pytest.mark.gpu
def test_a_table_too_small_sets_the_overflow_bit_and_the_wrapper_raises():
    from neuralnetworklibrary_amd import ops_text
    from neuralnetworklibrary_amd.Applications.Text import _split_corpus
    corpus = _split_corpus([['t%d' % i for i in range(100)]])
    toks = ops_text.token_bounds(corpus, ops_text.TEXT_MODE_SPLIT)
    keys = ops_text.token_hash(corpus, toks, ops_text.TEXT_SEEDS[0])
    table = ops_text.VocabTable(16)
    tok_slot = ops_text.vocab_insert(keys, toks.T, table)[:toks.T].tolist()     # returns: the probe loop ends after 16 steps
    assert int(table.status.item()) & ops_text.TEXT_STATUS_OVERFLOW
    assert sum(1 for s in tok_slot if s >= 0) == 16 and sum(1 for s in tok_slot if s == -1) == 84
    assert int((table.key != 0).sum().item()) == 16 and int(table.count.sum().item()) == 16
    with pytest.raises(RuntimeError, match='overflow'):
        ops_text.vocab_build(corpus, toks, ops_text.TEXT_SEEDS[0], cap=16)
    with pytest.raises(RuntimeError, match='overflow'):
        ops_text.text_numericalize(corpus, ops_text.TEXT_MODE_SPLIT, cap=16)


# ---- end to end -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('reverse', [False, True])
def test_text_dataset_from_strings_equals_the_restatement_chain(reverse):
    from neuralnetworklibrary_amd.Applications.Text import TextDataset, Tokenizer, numericalize, tokenize, tokenize_mp
    g = R.g26()
    texts = g['texts'] + ['Ünï-CODE stays: naïve café ÉCOLE', "I CAN'T EVEN.  It's 3.5/10 #fail<br />SOOOOO bad bad bad bad bad"]
    labels = ['pos' if i % 3 else 'neg' for i in range(len(texts))]
    tok = Tokenizer()
    assert tokenize(texts) == tokenize_mp(texts, ncpus=3) == [R.tokens(R.pre_rules(t)) for t in texts]
    assert tok.proc_text(texts[1]) == R.tokens(R.pre_rules(texts[1])) and tok.proc_texts([]) == []
    for max_vocab, min_freq in ((60000, 1), (60000, 2), (20, 1)):
        ds = TextDataset(texts, labels, reverse=reverse, tokenizer=tok, max_vocab=max_vocab, min_freq=min_freq)
        want, want_stoi = R.chain(texts, max_vocab, min_freq, reverse=reverse)
        assert list(ds.texts) == want and list(ds.stoi.items()) == list(want_stoi.items())
        assert ds.num_tokens == sum(len(t) for t in want) and len(ds) == len(texts)
        assert ds.label_dict == {'neg': 0, 'pos': 1} and list(ds.labels) == [ds.label_dict[l] for l in labels]
        ids, stoi = numericalize(tokenize(texts), max_vocab, min_freq)
        assert ([t[::-1] for t in ids] if reverse else ids) == want and stoi == ds.stoi
    # a train vocabulary reused for a second set
    train = TextDataset(texts[::2], labels[::2], reverse=reverse, tokenizer=tok, min_freq=2)
    second = TextDataset(texts[1::2], labels[1::2], train.stoi, reverse, tokenizer=tok)
    want, _ = R.chain(texts[1::2], stoi=train.stoi, reverse=reverse)
    assert list(second.texts) == want and second.stoi is train.stoi and any(0 in t for t in want)
    assert ds[1] == (ds.texts.iloc[1], ds.labels.iloc[1]) and ds[1][1] == 1


# ---- file routes ------------------------------------------------------------------------------------------------------------------

POS = ['I loved it, loved it a lot!', "GREAT movie, couldn't be better", 'loved the cast and the movie', 'a great great film<br />loved it']
NEG = ["I hated it, it's bad", 'BAD movie, really bad', 'hated the cast and the movie', 'a bad bad film -- hated it']


def _write_folders(root, n_rep=3):
    for split, rep in (('train', n_rep), ('val', 1)):
        for lab, texts in (('pos', POS), ('neg', NEG)):
            d = root / split / lab
            d.mkdir(parents=True)
            for r in range(rep):
                for i, t in enumerate(texts):
                    (d / ('%d_%d.txt' % (r, i))).write_bytes((t + ' take %d' % r).encode('utf-8'))
            (d / '._0_0.txt').write_bytes(b'\x00\x05resource fork')
            (d / 'notes.md').write_text('not a text file')
    (root / 'train' / 'pos' / 'z_latin1.txt').write_bytes(b'caf\xe9 loved')      # not UTF-8: decoded with errors='replace'
    flat = root / 'flat'
    flat.mkdir()
    for i, t in enumerate(POS + NEG):
        (flat / ('%02d.txt' % i)).write_text(t)


def _folder_texts(root, split, labels):
    texts, labs = [], []
    for lab in sorted(labels):
        d = root / split / lab
        for fn in sorted(os.listdir(d)):
            if fn.endswith('.txt') and not fn.startswith('._'):
                texts.append((d / fn).read_bytes().decode('utf-8', errors='replace'))
                labs.append(lab)
    return texts, labs


@pytest.mark.gpu
def test_datasets_from_text_files_and_csv(tmp_path):
    import pandas as pd
    from neuralnetworklibrary_amd.Applications.Text import TextDataset, Tokenizer
    _write_folders(tmp_path)
    tok = Tokenizer()
    texts, labs = _folder_texts(tmp_path, 'train', ['neg', 'pos'])
    assert len(texts) == 25 and '�' in texts[-1]
    want, want_stoi = R.chain(texts, min_freq=2)
    given = ['pos', 'neg']
    for labels in ('All', given):
        ds = TextDataset.from_text_files(str(tmp_path / 'train'), labels, tokenizer=tok, min_freq=2)
        assert list(ds.texts) == want and list(ds.stoi.items()) == list(want_stoi.items())
        assert ds.label_dict == {'neg': 0, 'pos': 1} and list(ds.labels) == [ds.label_dict[l] for l in labs]
    assert given == ['pos', 'neg']                                                # the caller's list is not sorted in place
    only = TextDataset.from_text_files(str(tmp_path / 'train'), ['pos'], ds.stoi, True, tokenizer=tok)
    assert list(only.texts) == R.chain(texts[12:], stoi=ds.stoi, reverse=True)[0] and only.label_dict == {'pos': 0}
    flat = TextDataset.from_text_files(str(tmp_path / 'flat') + '/', None, tokenizer=tok, min_freq=1)
    assert list(flat.texts) == R.chain(POS + NEG, min_freq=1)[0] and list(flat.labels) == [0] * 8 and flat.label_dict == {0: 0}
    csv = tmp_path / 'train.csv'
    pd.DataFrame({'text': POS + NEG, 'label': ['p'] * 4 + ['n'] * 4, 'other': range(8)}).to_csv(csv, index=False)
    a = TextDataset.from_csv(str(csv), 'text', 'label', tokenizer=tok, min_freq=1)
    assert list(a.texts) == R.chain(POS + NEG, min_freq=1)[0] and list(a.labels) == [1] * 4 + [0] * 4
    b = TextDataset.from_csv(str(csv), 'text', None, a.stoi, True, tokenizer=tok)
    assert list(b.texts) == R.chain(POS + NEG, stoi=a.stoi, reverse=True)[0] and list(b.labels) == [0] * 8


@pytest.mark.gpu
def test_data_objects_from_files_train_a_step_and_generate(tmp_path):
    import pandas as pd
    from neuralnetworklibrary_amd.Applications.Text import (LanguageModelDataObj, LanguageModelNet, RegSeqCrossEntropyLoss,
                                                            TextClassificationDataObj, TextClassificationNet, Tokenizer)
    from neuralnetworklibrary_amd.General.Learner import Learner
    torch.manual_seed(0)
    np.random.seed(0)
    _write_folders(tmp_path)
    tok = Tokenizer()
    bs = 4
    data = TextClassificationDataObj.from_folders(bs, ['neg', 'pos'], str(tmp_path / 'train'), str(tmp_path / 'val'), tokenizer=tok, min_freq=2,
                                                  num_workers=0)
    texts, _ = _folder_texts(tmp_path, 'train', ['neg', 'pos'])
    assert list(data.stoi.items()) == list(R.chain(texts, min_freq=2)[1].items()) and data.val_ds.stoi is data.stoi
    assert len(data.train_ds) == 25 and len(data.val_ds) == 8 and data.test_ds is None
    x, y = next(iter(data.train_dl))
    assert x.dtype == torch.int64 and x.shape[0] == bs and y.shape == (bs,) and int(x.max()) < len(data.stoi)
    lm = LanguageModelNet(data, emb_dim=32, hidden_size=64, num_layers=2)
    net = TextClassificationNet(str(tmp_path), lm, 2, attn_size=16, fc_layer_sizes=[16], fc_drops=[0.1, 0.1])
    learner = Learner(str(tmp_path), data, net, optimizer='Adam', loss_func=RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(clip=1.0)
    net.train()
    loss = learner.train1minibatch(x.cuda(), y.cuda(), [3e-3, 3e-3, 3e-3], betas_batch=(0.7, 0.99))
    assert np.isfinite(float(loss))

    csv = tmp_path / 'lm.csv'
    pd.DataFrame({'text': (POS + NEG) * 6}).to_csv(csv, index=False)
    np.random.seed(1)
    lmd = LanguageModelDataObj.from_csv(2, 5, str(csv), tokenizer=tok, min_freq=2)
    assert lmd.target_type == 'lang_model' and lmd.test_ds is None and len(lmd.train_ds) + len(lmd.val_ds) == 48
    xb, yb = next(iter(lmd.train_dl))
    assert xb.shape == yb.shape and xb.shape[0] == 2 and torch.equal(xb[:, 1:], yb[:, :-1])
    net = LanguageModelNet(lmd, emb_dim=32, hidden_size=64, num_layers=2).to('cuda')
    out = net.predict_from_string("I LOVED the movie, didn't you?", 2, tokenize=Tokenizer().proc_text)
    assert isinstance(out, str) and len(out.split(' ')) == len(R.tokens("I LOVED the movie, didn't you?")) + 2
