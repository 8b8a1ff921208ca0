"""Text application of the drop-in API: the model / loss side of the reference's Applications/Text.py
(§3 models :441-752, §4 losses :754-808) plus the language-model batch loader (:231-332).

HIP-backed hot path (K5/K5b): the embedding gather with vocabulary-row dropout (ops.embedding_rowmask), every LSTM
layer (ops.lstm_layer: one fp32-MFMA GEMM for all input projections + the recurrence kernels, BPTT in C), the tied
decoder GEMM (ops.linear) and the fused softmax-cross-entropy over the vocabulary (ops.cross_entropy_nd).
Same classes, constructor arguments, state_dict keys (enc.word_embed.embed.weight, enc.lstms.{l}.lstm.{weight_ih_l0,
bias_ih_l0,bias_hh_l0,weight_hh_l0_raw}, dec.lin.weight tied) and quirks as the reference: hidden dropout is applied
after EVERY LSTM layer including the last (Text.py:546), hidden state is carried (detached) across batches and never
reset by the Learner (Text.py:547-550).  Text generation (K5d, Text.py:655-676): LanguageModelNet.predict_from_tokens /
predict_from_string on ops_text.LstmCellB1 and ops_text.LmNextToken (batch 1, one timestep, nothing read back inside the loop).
Tokenisation / numericalisation (:19-229) is partly built (K17): `Tokenizer`, `tokenize`, `tokenize_mp`,
`numericalize` and the string / file routes of the datasets run on the HIP tokeniser and vocabulary kernels of
csrc/text_tokens.hip with the package's OWN byte grammar (see `Tokenizer`), opted into with the keyword-only `tokenizer=`
argument; spaCy itself, corpora of 2^31 bytes or more, a parallel host pre-rule pass, ids kept resident for the LM loader and the
wt103 vocabulary are not built.
"""
import math
import os
import re

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..General.Core import *          # noqa: F401,F403
from ..General.Layers import *        # noqa: F401,F403
from ..General.Learner import *       # noqa: F401,F403
from ..General.LossesMetrics import * # noqa: F401,F403
from ..General.Optimizer import *     # noqa: F401,F403
from ..General.Core import TEN, SplitTrainVal, correct_foldername, default_device, list_mult, separate_bn_layers
from ..General.Layers import FullyConnectedNet
from .. import ops, ops_text
from ..dist import keyed_mask


# ---- tokenisation and numericalisation (Text.py:19-122) on the HIP tokeniser (K17) ------------------------------------------------

class Tokenizer(object):
    """The reference's Tokenizer (Text.py:28-75) without spaCy: host pre-rules on the Python string, then the package's OWN byte
    grammar on the device (csrc/text_tokens.hip, csrc/text_grammar.h).  `lang` is accepted and ignored.  Nothing is printed.

    Host pre-rules, in this order (they change a text's length, so they run as re.sub before the upload): (1) re_rep: a
    non-space character repeated 4 times or more -> ' tk_rep <n> <c> '; (2) re_word_rep: a word (with what separates it from the next)
    repeated 4 times or more -> ' tk_wrep <n> <word> '; (3) <br /> -> newline; (4) '/' and '#' get a space on either side.  The
    reference applies do_caps between (2) and (4) and (3) last; (3) and (4) commute with the case rule below: `br` has 2 letters and
    never gets t_up, and '/' and '#' are not word bytes.

    The grammar, over the UTF-8 bytes of ONE text (no token crosses a text boundary, no rule looks across one).  Byte classes:
    S = 0x09-0x0D and 0x20; W = 0-9 A-Z a-z _ and every byte >= 0x80 (multibyte characters are word characters and are never
    cased); P = everything else; a '.' or ',' whose two neighbours are both ASCII digits counts as W (3.5 and 1,000 stay whole).
      * A maximal run of W bytes is a token.
      * A maximal run of one repeated P byte is a token: ... -- !!
      * S separates tokens and is never a token (spaCy emits whitespace tokens; this grammar does not).
      * An apostrophe with a letter, digit or _ (a W byte proper) on both sides starts a token that runs through the following W
        run: 's 're 'll.  If the byte before it is n / N and the run after it is exactly t / T, the token is n't and the word
        before ends one byte earlier: don't -> do, n't; n't alone -> n't.
      * <eos>, <bos>, <unk> (lower case) are single tokens and take precedence over every other rule.
    Whether a token starts at a byte depends on at most 5 bytes before it and 4 after it; nothing is sequential.
    Case rule (do_caps, Text.py:58-67, restricted to ASCII): if a token begins a maximal run of letters, digits, _ and bytes >= 0x80
    (the digit rule does not extend this run, and it may reach past the token: DON'T) that is longer than 2 bytes and has at least
    one A-Z and no a-z, the pseudo-token t_up precedes the token.  Every token is compared, hashed and returned with A-Z lowered.
    Mode `split` (numericalize on already tokenised input): tokens are maximal runs of non-S bytes; no case rule, no lowering.

    Deliberate differences from the reference: no whitespace tokens; only ASCII letters are cased; no spaCy exceptions list (only
    the contraction rules above); an all-capitals run that begins INSIDE a token ('CLOCK in O'CLOCK, 5AB in 3.5AB) gets no t_up and
    does not split the token, where do_caps' inserted spaces would; nothing is printed; tokenize_mp's `ncpus` is ignored."""

    re_br = re.compile(r'<\s*br\s*/?>', re.IGNORECASE)
    re_rep = re.compile(r'(\S)(\1{3,})')
    re_word_rep = re.compile(r'(\b\w+\W+)(\1{3,})')
    re_slash_hash = re.compile(r'([/#])')

    def __init__(self, lang='en'):
        self.lang = lang

    def sub_br(self, x):
        return self.re_br.sub('\n', x)

    @staticmethod
    def replace_rep(m):
        c, rest = m.groups()
        return ' tk_rep %d %s ' % (len(rest) + 1, c)

    @staticmethod
    def replace_wrep(m):
        w, rest = m.groups()
        return ' tk_wrep %d %s ' % (len(rest.split()) + 1, w)

    def pre_rules(self, s):
        "the four host rules on one text, in the order of the class docstring"
        s = self.re_rep.sub(Tokenizer.replace_rep, s)
        s = self.re_word_rep.sub(Tokenizer.replace_wrep, s)
        return self.re_slash_hash.sub(r' \1 ', self.sub_br(s))

    def corpus(self, ss):
        "pre-rules on every text, then ONE upload: the ops_text.TextCorpus the kernels read (ValueError from 2^31 bytes on)"
        return ops_text.TextCorpus.from_texts([self.pre_rules(s).encode('utf-8', 'surrogateescape') for s in ss])

    def proc_text(self, s):
        "one text -> its token strings"
        return self.proc_texts([s])[0]

    def proc_texts(self, ss):
        "texts -> token-string lists: one upload, one pass of the token kernels, one copy back of the token records"
        ss = list(ss)
        if not ss:
            return []
        corpus = self.corpus(ss)
        return ops_text.token_strings(corpus, ops_text.token_bounds(corpus, ops_text.TEXT_MODE_GRAMMAR))


def tokenize(ss):
    "token-string lists of the texts ss (Text.py:77-83), through Tokenizer().proc_texts"
    return Tokenizer().proc_texts(ss)


def tokenize_mp(ss, ncpus=None):
    "as tokenize (Text.py:85-93); `ncpus` is accepted and ignored: there is no process pool, the texts go through the device in one pass"
    return Tokenizer().proc_texts(ss)


def _split_corpus(ss):
    "already tokenised texts as a corpus for the `split` mode: tokens joined by one space; a token the mode would cut or lose raises"
    texts = []
    for toks in ss:
        enc = [t.encode('utf-8', 'surrogateescape') for t in toks]
        for t, b in zip(toks, enc):
            if not b or len(b.split()) != 1 or len(b.split()[0]) != len(b):
                raise ValueError('numericalize: token %r is empty or contains whitespace (0x09-0x0D, 0x20)' % (t,))
        texts.append(b' '.join(enc))
    return ops_text.TextCorpus.from_texts(texts)


def numericalize(ss, max_vocab=60000, min_freq=6, stoi=None):
    """(ss_numeric, stoi) for lists of token strings (Text.py:95-122), on the device through the `split` mode: without `stoi` the
    vocabulary is the max_vocab most common tokens (ties in order of first occurrence) that then occur at least min_freq times,
    after _unk_ _pad_ _bos_ _eos_; with `stoi`, tokens it lacks give 0.  Nothing is printed."""
    ss = [list(toks) for toks in ss]
    if not ss:
        return [], (stoi if stoi is not None else {s: i for i, s in enumerate(ops_text.TEXT_SPECIALS)})
    out = ops_text.text_numericalize(_split_corpus(ss), ops_text.TEXT_MODE_SPLIT, max_vocab, min_freq, stoi)
    return out.lists(), out.stoi


# ---- data: datasets (Text.py:127-229) -------------------------------------------------------------------------------

_NO_TOKENIZER = ('tokenisation (spaCy) is not part of this package (SURVEY.md §2.1 row 14): pass token-id lists, e.g. what the '
                 "reference's numericalize() returns")


class TextDataset(object):
    """Texts + labels for language modelling and text classification (Text.py:127-187).  Same attributes as the reference: texts /
    labels as pandas Series, the sorted label_dict, num_tokens.

    tokenizer=None (default): `texts` are token-id lists (what the reference computes from strings with tokenize_mp + numericalize);
    strings raise NotImplementedError; `stoi` is kept as given.
    tokenizer=Tokenizer(): `texts` are strings and the fused route runs: the tokenizer's host pre-rules, one upload, the kernels of
    csrc/text_tokens.hip (token bounds, then the vocabulary built from these texts with max_vocab / min_freq — or the lookup in a given
    `stoi` — and the ids, reversed per text on the device if `reverse`), one copy back of ids and offsets.  Token strings are never
    materialised on the host, apart from the vocabulary; the result equals numericalize(tokenize(texts), max_vocab, min_freq, stoi)."""

    def __init__(self, texts, labels, stoi=None, reverse=False, *, tokenizer=None, max_vocab=60000, min_freq=6):
        import pandas as pd
        texts = list(texts)
        self.reverse = reverse
        if tokenizer is not None:
            if not all(isinstance(t, str) for t in texts):
                raise TypeError('TextDataset: with a tokenizer every text must be a string')
            if texts:
                out = ops_text.text_numericalize(tokenizer.corpus(texts), ops_text.TEXT_MODE_GRAMMAR, max_vocab, min_freq, stoi, reverse)
                self.stoi, ids = out.stoi, out.lists()
            else:
                self.stoi, ids = (stoi if stoi is not None else {s: i for i, s in enumerate(ops_text.TEXT_SPECIALS)}), []
            self.texts = pd.Series(ids, dtype=object)
        else:
            if any(isinstance(t, str) for t in texts):
                raise NotImplementedError(_NO_TOKENIZER)
            self.stoi = stoi
            self.texts = pd.Series([[int(v) for v in t] for t in texts], dtype=object)
            if reverse:
                self.texts = pd.Series([list(reversed(t)) for t in self.texts], dtype=object)
        self.num_tokens = sum(len(t) for t in self.texts)
        unique_labels = sorted(list(set(labels)))
        self.label_dict = {lab: i for i, lab in enumerate(unique_labels)}
        self.labels = pd.Series([self.label_dict[lab] for lab in labels], dtype=np.int64)

    def __len__(self):
        return len(self.texts)

    def __getitem__(self, idx):
        return self.texts.iloc[idx], self.labels.iloc[idx]

    def split_train_val(self):
        "(train, val) datasets split by General.Core.SplitTrainVal (20 % validation, np.random) — Text.py:160-181"
        import copy
        all_texts, all_labels = copy.deepcopy(self.texts), copy.deepcopy(self.labels)
        train_ds, val_ds = self, copy.deepcopy(self)
        train_idxs, val_idxs = SplitTrainVal(list(range(len(self.texts))))
        for ds, idxs in ((train_ds, train_idxs), (val_ds, val_idxs)):
            ds.texts = all_texts[idxs]
            ds.texts.index = range(len(ds.texts))
            ds.labels = all_labels[idxs]
            ds.labels.index = range(len(ds.labels))
            ds.num_tokens = sum(len(t) for t in ds.texts)
        return train_ds, val_ds

    @classmethod
    def from_csv(cls, csv_file, text_col, label_col=None, stoi=None, reverse=False, *, tokenizer=None, max_vocab=60000, min_freq=6):
        "one text per csv row, labels from `label_col` or all 0 (Text.py:180-187); needs a tokenizer"
        if tokenizer is None:
            raise NotImplementedError(_NO_TOKENIZER)
        import pandas as pd
        df = pd.read_csv(csv_file)
        labels = list(df[label_col]) if label_col else [0] * len(df)
        return cls([str(t) for t in df[text_col]], labels, stoi, reverse, tokenizer=tokenizer, max_vocab=max_vocab, min_freq=min_freq)

    @classmethod
    def from_text_files(cls, folder, labels, stoi=None, reverse=False, *, tokenizer=None, max_vocab=60000, min_freq=6):
        """.txt files of `folder` (labels=None: all labelled 0), of each of its sub-folders (labels='All') or of the sub-folders named
        in the list `labels`, the sub-folder's name being the label (Text.py:189-229); needs a tokenizer.  Deliberate differences from
        the reference, as on the image side (Vision.py's from_folders): every listing is SORTED (os.listdir's order is the file
        system's), files whose name starts with '._' are skipped, files are read as bytes, decoded as UTF-8 with errors='replace',
        and closed, and the caller's `labels` list is not sorted in place."""
        if tokenizer is None:
            raise NotImplementedError(_NO_TOKENIZER)
        folder = correct_foldername(folder)

        def read_all(sub):
            names = sorted(fn for fn in os.listdir(folder + sub) if fn.endswith('.txt') and not fn.startswith('._'))
            out = []
            for fn in names:
                with open(os.path.join(folder + sub, fn), 'rb') as f:
                    out.append(f.read().decode('utf-8', errors='replace'))
            return out

        if labels is None:
            texts = read_all('')
            text_labels = [0] * len(texts)
        else:
            if isinstance(labels, str):
                labels = [d for d in os.listdir(folder) if os.path.isdir(folder + d)]
            texts, text_labels = [], []
            for lab in sorted(labels):
                got = read_all(lab)
                texts += got
                text_labels += [lab] * len(got)
        return cls(texts, text_labels, stoi, reverse, tokenizer=tokenizer, max_vocab=max_vocab, min_freq=min_freq)


# ---- data: text-classification batches (Text.py:334-440) -----------------------------------------------------------

class TextLengthSampler(torch.utils.data.Sampler):
    """Batches of similar-length texts (Text.py:334-381).  Sorts `ds` by text length, longest first, IN PLACE (ds.texts,
    ds.labels re-ordered, ds.perm = the permutation: predictions of an unshuffled loader line up with the permuted labels),
    then cuts groups of bs*bpg consecutive texts.  random=True: every pass shuffles the order of the groups after the first
    (which stays first: the longest batch comes first) and the texts within each group, with np.random — including the pass
    that counts the batches in the constructor, as in the reference."""

    def __init__(self, ds, bs, bpg=10, random=False):
        L = len(ds)
        perm = list(range(L))
        perm.sort(key=lambda i: len(ds.texts[i]), reverse=True)
        ds.texts, ds.labels, ds.perm = ds.texts[perm], ds.labels[perm], perm
        ds.texts.index, ds.labels.index = range(L), range(L)
        group_sz = bs * bpg
        self.groups = [list(range(i, min(i + group_sz, L))) for i in range(0, L, group_sz)]
        self.bs, self.random = bs, random
        self.length = len([x for x in self])

    def __len__(self):
        return self.length

    def __iter__(self):
        if self.random:
            groups = self.groups[1:]
            np.random.shuffle(groups)
            self.groups = [self.groups[0]] + groups
        for g in self.groups:
            if self.random:
                np.random.shuffle(g)
            for i in range(0, len(g), self.bs):
                yield g[i:min(i + self.bs, len(g))]


class TextLengthCollater(object):
    "Pads every text of a batch at the end to the batch's longest; CPU int64 tensors (x [bs, seqlen], y [bs]) — Text.py:383-395"

    def __init__(self, pad_token):
        self.pad_token = pad_token

    def __call__(self, batch):
        texts, labels = [list(b[0]) for b in batch], [b[1] for b in batch]
        m = max(len(t) for t in texts)
        x = np.array([t + [self.pad_token] * (m - len(t)) for t in texts], dtype=np.int64)
        return TEN(x, GPU=False), TEN(np.array(labels, dtype=np.int64), GPU=False)


class TextClassificationDataObj(object):
    """train / val / (test) loaders of length-bucketed, end-padded batches, target_type 'text_classify' (Text.py:397-440).
    The train sampler shuffles (random=True), val / test keep the longest-first order."""

    def __init__(self, train_ds, val_ds, test_ds, bs, bpg=10, num_workers=6):
        from torch.utils.data import DataLoader
        self.bs, self.stoi, self.target_type = bs, train_ds.stoi, 'text_classify'
        self.train_ds, self.val_ds, self.test_ds = train_ds, val_ds, test_ds
        collater = TextLengthCollater(self.stoi['_pad_'])
        sampler_train = TextLengthSampler(train_ds, bs, bpg, random=True)
        sampler_val = TextLengthSampler(val_ds, bs, bpg, random=False)
        if test_ds:
            sampler_test = TextLengthSampler(test_ds, bs, bpg, random=False)
        self.train_dl = DataLoader(train_ds, collate_fn=collater, batch_sampler=sampler_train, num_workers=num_workers)
        self.val_dl = DataLoader(val_ds, collate_fn=collater, batch_sampler=sampler_val, num_workers=num_workers)
        if test_ds:
            self.test_dl = DataLoader(test_ds, collate_fn=collater, batch_sampler=sampler_test, num_workers=num_workers)

    @classmethod
    def from_csv(cls, bs, csv_train, csv_val=None, csv_test=None, text_col='text', label_col='label', reverse=False, stoi=None, *,
                 tokenizer=None, max_vocab=60000, min_freq=6, bpg=10, num_workers=6):
        "csv files -> data object (Text.py:411-424): the vocabulary comes from the train file; without csv_val the train set is split"
        if tokenizer is None:
            raise NotImplementedError(_NO_TOKENIZER)
        train_ds = TextDataset.from_csv(csv_train, text_col, label_col, stoi, reverse, tokenizer=tokenizer, max_vocab=max_vocab, min_freq=min_freq)
        stoi = train_ds.stoi
        if csv_val:
            val_ds = TextDataset.from_csv(csv_val, text_col, label_col, stoi, reverse, tokenizer=tokenizer)
        else:
            train_ds, val_ds = train_ds.split_train_val()
        test_ds = TextDataset.from_csv(csv_test, text_col, label_col, stoi, reverse, tokenizer=tokenizer) if csv_test else None
        return cls(train_ds, val_ds, test_ds, bs, bpg, num_workers)

    @classmethod
    def from_folders(cls, bs, labels, train, val=None, test=None, reverse=False, stoi=None, *, tokenizer=None, max_vocab=60000, min_freq=6, bpg=10, num_workers=6):
        "folders of .txt files in label sub-folders -> data object (Text.py:426-438); `labels` as in TextDataset.from_text_files"
        if tokenizer is None:
            raise NotImplementedError(_NO_TOKENIZER)
        train_ds = TextDataset.from_text_files(train, labels, stoi, reverse, tokenizer=tokenizer, max_vocab=max_vocab, min_freq=min_freq)
        stoi = train_ds.stoi
        if val:
            val_ds = TextDataset.from_text_files(val, labels, stoi, reverse, tokenizer=tokenizer)
        else:
            train_ds, val_ds = train_ds.split_train_val()
        test_ds = TextDataset.from_text_files(test, labels, stoi, reverse, tokenizer=tokenizer) if test else None
        return cls(train_ds, val_ds, test_ds, bs, bpg, num_workers)


# ---- data: language-model batches (Text.py:231-332) ----------------------------------------------------------------

class LanguageModelDataLoader(object):
    """All texts concatenated, split into bs parallel streams [bs, seqlen+1]; yields consecutive (x, y) windows of
    `bptt` tokens (train: 5 % of batches halved, minus U{0..9} jitter), y = x shifted by one (Text.py:231-290).
    `ds` needs `.texts` (sequence of token-id lists, or a pandas Series) and `.num_tokens`.
    device_resident=True (MI355X addition): the `[bs, seqlen+1]` token matrix is uploaded once per epoch
    and the (x, y) windows are device slices — no per-step numpy -> tensor -> H2D copy."""

    def __init__(self, ds, bs, bptt, random=True, device_resident=False):
        self.bs, self.bptt, self.random, self.device_resident = bs, bptt, random, device_resident
        self.texts, self.ntexts = ds.texts, len(ds.texts)
        self.seqlen = (ds.num_tokens // bs) - 1
        self.ntoks = bs * (self.seqlen + 1)
        self.concat_texts()
        self.set_batch_lengths()

    def _text(self, i):
        return self.texts.iloc[i] if hasattr(self.texts, 'iloc') else self.texts[i]

    def concat_texts(self):
        idxs = list(range(self.ntexts))
        if self.random:
            np.random.shuffle(idxs)
        flat = np.concatenate([np.asarray(self._text(i), dtype=np.int64) for i in idxs])[:self.ntoks]
        self.combined_text = flat.reshape(self.bs, self.seqlen + 1)
        self.combined_dev = TEN(self.combined_text) if self.device_resident else None

    def set_batch_lengths(self):
        self.batch_lengths = []
        i, used = 0, 0
        while used < self.seqlen:
            bptt = self.bptt
            if self.random and i > 0 and np.random.random() < 0.05:
                bptt = bptt // 2
            if self.random and i > 0:
                bptt = bptt - np.random.randint(0, 10)
            n = min(self.seqlen - used, bptt)
            used += n
            i += 1
            self.batch_lengths.append(n)

    def __len__(self):
        return len(self.batch_lengths)

    def __iter__(self):
        used = 0
        for bl in self.batch_lengths:
            if self.combined_dev is not None:
                yield (self.combined_dev[:, used:used + bl].contiguous(), self.combined_dev[:, used + 1:used + bl + 1].contiguous())
            else:
                yield (TEN(self.combined_text[:, used:used + bl]), TEN(self.combined_text[:, used + 1:used + bl + 1]))
            used += bl
        if self.random:
            self.concat_texts()


class LanguageModelDataObj(object):
    "train / val / (test) LanguageModelDataLoaders, target_type 'lang_model' (Text.py:292-304)"

    def __init__(self, train_ds, val_ds, test_ds, bs, bptt, device_resident=False):
        self.bs, self.bptt, self.stoi, self.target_type = bs, bptt, train_ds.stoi, 'lang_model'
        self.train_ds, self.val_ds, self.test_ds = train_ds, val_ds, test_ds
        self.train_dl = LanguageModelDataLoader(train_ds, bs, bptt, True, device_resident)
        self.val_dl = LanguageModelDataLoader(val_ds, bs, bptt, False, device_resident)
        if test_ds:
            self.test_dl = LanguageModelDataLoader(test_ds, bs, bptt, False, device_resident)

    @classmethod
    def from_csv(cls, bs, bptt, csv_train, csv_val=None, csv_test=None, text_col='text', reverse=False, *, tokenizer=None,
                 max_vocab=60000, min_freq=6, device_resident=False):
        "csv files with one text per row -> data object (Text.py:306-318); the vocabulary comes from the train file"
        if tokenizer is None:
            raise NotImplementedError(_NO_TOKENIZER)
        train_ds = TextDataset.from_csv(csv_train, text_col, None, None, reverse, tokenizer=tokenizer, max_vocab=max_vocab, min_freq=min_freq)
        stoi = train_ds.stoi
        if csv_val:
            val_ds = TextDataset.from_csv(csv_val, text_col, None, stoi, reverse, tokenizer=tokenizer)
        else:
            train_ds, val_ds = train_ds.split_train_val()
        test_ds = TextDataset.from_csv(csv_test, text_col, None, stoi, reverse, tokenizer=tokenizer) if csv_test else None
        return cls(train_ds, val_ds, test_ds, bs, bptt, device_resident)

    @classmethod
    def from_folders(cls, bs, bptt, labels, train, val=None, test=None, reverse=False, *, tokenizer=None, max_vocab=60000, min_freq=6,
                     device_resident=False):
        "folders of .txt files -> data object (Text.py:320-332); `labels` as in TextDataset.from_text_files"
        if tokenizer is None:
            raise NotImplementedError(_NO_TOKENIZER)
        train_ds = TextDataset.from_text_files(train, labels, None, reverse, tokenizer=tokenizer, max_vocab=max_vocab, min_freq=min_freq)
        stoi = train_ds.stoi
        if val:
            val_ds = TextDataset.from_text_files(val, labels, stoi, reverse, tokenizer=tokenizer)
        else:
            train_ds, val_ds = train_ds.split_train_val()
        test_ds = TextDataset.from_text_files(test, labels, stoi, reverse, tokenizer=tokenizer) if test else None
        return cls(train_ds, val_ds, test_ds, bs, bptt, device_resident)


# ---- models --------------------------------------------------------------------------------------------------------

class LockedDropout(nn.Module):
    "One dropout mask [1, bs, C] shared by every timestep of x [T, bs, C] (Text.py:443-452)"

    def __init__(self, drop):
        super().__init__()
        self.drop = nn.Dropout(drop)

    def forward(self, x, mask=None):
        if mask is None and self.training and self.drop.p > 0:
            mask = keyed_mask((1, x.size(1), x.size(2)), self.drop.p, x.device, sample_dim=1)      # None unless use_keyed_dropout()
        if mask is None:
            mask = self.drop(torch.ones(1, x.size(1), x.size(2), device=x.device))
        return mask * x


class EmbeddingDropout(nn.Module):
    "Word embedding with whole-row (per vocabulary entry) dropout, then locked dropout (Text.py:454-475)"

    def __init__(self, vocab_size, emb_dim, drop1, drop2, pad_token):
        super().__init__()
        self.vocab_size, self.pad_token = vocab_size, pad_token
        self.drop1, self.drop2 = nn.Dropout(drop1), LockedDropout(drop2)
        self.embed = nn.Embedding(vocab_size, emb_dim, pad_token)
        nn.init.uniform_(self.embed.weight, -0.1, 0.1)
        with torch.no_grad():
            self.embed.weight[pad_token].zero_()

    def forward(self, x, row_mask=None, locked_mask=None):
        # x: [seqlen, bs] -> [seqlen, bs, emb_dim]
        if not self.training:
            return ops.embedding_rowmask(x, self.embed.weight, None, self.pad_token)
        if row_mask is None and self.drop1.p > 0:
            row_mask = keyed_mask((self.vocab_size, 1), self.drop1.p, x.device)     # parameter-shaped: the same on every rank
        if row_mask is None:
            row_mask = self.drop1(torch.ones(self.vocab_size, 1, device=x.device))
        out = ops.embedding_rowmask(x, self.embed.weight, row_mask, self.pad_token)
        return self.drop2(out, locked_mask)


class _LSTMParams(nn.Module):
    """Parameter holder with nn.LSTM's names and init (uniform(-1/sqrt(H), 1/sqrt(H))) in the order the reference ends
    up with after clear_non_raw(): weight_ih_l0, bias_ih_l0, bias_hh_l0, weight_hh_l0_raw (Text.py:486-493)."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        k = 1.0 / math.sqrt(hidden_size)
        mk = lambda *s: nn.Parameter(torch.empty(*s).uniform_(-k, k))
        self.weight_ih_l0 = mk(4 * hidden_size, input_size)
        self.bias_ih_l0 = mk(4 * hidden_size)
        self.bias_hh_l0 = mk(4 * hidden_size)
        self.weight_hh_l0_raw = mk(4 * hidden_size, hidden_size)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # reference checkpoints saved before clear_non_raw() also carry `weight_hh_l0` (the same tensor): ignore it
        state_dict.pop(prefix + 'weight_hh_l0', None)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class WeightDropLSTM1(nn.Module):
    """Single-layer LSTM whose hidden-to-hidden matrix gets elementwise dropout (one mask per forward call, shared by
    all timesteps) — Text.py:477-513."""

    nnl_stateful_forward = True        # the weight-drop seed of a call is drawn on the host (ops_text.lstm_layer): not replayable

    def __init__(self, input_size, hidden_size, drop):
        super().__init__()
        self.weight_drop = nn.Dropout(drop)
        self.lstm = _LSTMParams(input_size, hidden_size)

    def setup_raw(self):
        pass

    def clear_non_raw(self):
        pass          # there is no non-raw copy to clear: weight_hh_l0_raw is the only recurrent parameter

    def forward(self, x, h0c0, weight_mask=None):
        p = self.lstm
        if weight_mask is None and self.training and self.weight_drop.p > 0:
            weight_mask = keyed_mask(p.weight_hh_l0_raw.shape, self.weight_drop.p, p.weight_hh_l0_raw.device)   # None unless keyed
        # W = Dropout_p(W_raw) (Text.py:511) is applied INSIDE the layer: one pass that also pads W for the recurrence kernels
        drop_p = self.weight_drop.p if (self.training and weight_mask is None) else 0.0
        return ops.lstm_layer(x, h0c0[0], h0c0[1], p.weight_ih_l0, p.weight_hh_l0_raw, p.bias_ih_l0, p.bias_hh_l0,
                              weight_mask=weight_mask, weight_p=drop_p)


class LSTM_Encoder(nn.Module):
    """Embedding dropout -> num_layers x (WeightDropLSTM1 -> locked hidden dropout), carried hidden state
    (Text.py:515-551).  `fixed_masks` (dict with 'emb_rows', 'emb_locked', 'weights'[l], 'hidden'[l]) pins the dropout
    masks for parity tests."""

    nnl_stateful_forward = True        # carries (h, c) between minibatches on the Python side: Learner.use_graphs() keeps such steps eager

    def __init__(self, vocab_size, emb_dim, hidden_size, num_layers, pad_token, drops, bs):
        super().__init__()
        emb_drop1, emb_drop2, weight_drop, hidden_drop = drops
        self.word_embed = EmbeddingDropout(vocab_size, emb_dim, emb_drop1, emb_drop2, pad_token)
        self.hidden_drop = LockedDropout(hidden_drop)
        self.sizes = [emb_dim] + (num_layers - 1) * [hidden_size] + [emb_dim]
        self.lstms = nn.ModuleList([WeightDropLSTM1(self.sizes[i], self.sizes[i + 1], weight_drop) for i in range(num_layers)])
        self.fixed_masks = None
        self.reset(bs)

    def reset(self, bs):
        dev = self.word_embed.embed.weight.device
        self.h = [torch.zeros(1, bs, self.sizes[i], device=dev) for i in range(1, len(self.sizes))]
        self.c = [torch.zeros(1, bs, self.sizes[i], device=dev) for i in range(1, len(self.sizes))]

    def forward(self, x):
        # x: [bs, seqlen] -> [seqlen, bs, emb_dim]
        fm = self.fixed_masks or {}
        dev = self.word_embed.embed.weight.device
        if self.h[0].device != dev:
            self.h, self.c = [t.to(dev) for t in self.h], [t.to(dev) for t in self.c]
        x = self.word_embed(x.transpose(1, 0), fm.get('emb_rows'), fm.get('emb_locked'))
        h_n, c_n = [], []
        for i, lstm in enumerate(self.lstms):
            wm = fm['weights'][i] if 'weights' in fm else None
            x, (hn, cn) = lstm(x, (self.h[i], self.c[i]), wm)
            x = self.hidden_drop(x, fm['hidden'][i] if 'hidden' in fm else None)     # also after the last layer (:546)
            h_n.append(hn.detach())
            c_n.append(cn.detach())
        self.h, self.c = h_n, c_n
        return x


class LanguageModelDecoder(nn.Module):
    "Locked dropout -> tied linear -> [bs, vocab, seqlen] (Text.py:553-573)"

    def __init__(self, vocab_size, emb_dim, drop, tied_weight):
        super().__init__()
        self.lin = nn.Linear(emb_dim, vocab_size, bias=False)
        self.drop = LockedDropout(drop)
        self.lin.weight = tied_weight
        self.fixed_mask = None

    def forward(self, enc_out):
        pred = ops.linear(self.drop(enc_out, self.fixed_mask), self.lin.weight, None)      # [seq, bs, V]
        return pred.permute(1, 2, 0), enc_out


class TextClassificationDecoder(nn.Module):
    "Attention pooling over encoder outputs -> FullyConnectedNet (Text.py:575-609)"

    def __init__(self, emb_dim, num_classes, attn_size, fc_layer_sizes, fc_drops):
        super().__init__()
        self.fc = FullyConnectedNet([emb_dim] + fc_layer_sizes + [num_classes], fc_drops)
        self.attn1 = nn.Linear(emb_dim, attn_size)
        self.attn2 = nn.Linear(attn_size, 1)
        for m in (self.attn1, self.attn2):
            nn.init.kaiming_normal_(m.weight)
            nn.init.constant_(m.bias, 0)

    def forward(self, enc_in, enc_out):
        attn = ops.linear(enc_out, self.attn1.weight, self.attn1.bias, relu=True)       # seqlen x bs x attn_size
        if enc_out.dim() == 3 and enc_out.shape[0] > 1 and enc_out.shape[1] > 1:
            # attn2 -> softmax -> pad mask -> renormalise -> weighted sum in one HIP kernel each way (ops_text.attention_pool)
            attn, combined = ops_text.attention_pool(attn, self.attn2.weight, self.attn2.bias, enc_out, enc_in, 1)
            return self.fc(combined), attn
        # seqlen 1 or bs 1: the reference's .squeeze() drops that dimension too, and what follows broadcasts accordingly
        attn = ops.linear(attn, self.attn2.weight, self.attn2.bias).squeeze()          # seqlen x bs
        attn = F.softmax(attn, dim=0)
        attn = attn * (enc_in.transpose(1, 0) != 1).float()                            # ignore the pad token
        attn = attn / attn.sum(dim=0).unsqueeze(0)
        combined = (attn.unsqueeze(2) * enc_out).sum(0)                                # bs x emb_dim
        return self.fc(combined), attn


class _Vocab:
    "minimal stand-in for a data object: stoi + bs"
    def __init__(self, stoi, bs):
        self.stoi, self.bs = stoi, bs


class LanguageModelNet(nn.Module):
    """AWD-LSTM language model: LSTM_Encoder (400 / 1150 / 3 layers) + tied LanguageModelDecoder (Text.py:611-702).
    `pretrained` weights (wt103) are LFS blobs absent from the reference snapshot -> only None is supported here."""

    def __init__(self, data, enc_drops=[0.05, 0.25, 0.2, 0.15], dec_drop=0.1, drop_scaling=0.7, pretrained=None,
                 emb_dim=400, hidden_size=1150, num_layers=3):
        super().__init__()
        enc_drops, dec_drop = list_mult(list(enc_drops), drop_scaling), dec_drop * drop_scaling
        vocab_size, pad_token = len(data.stoi), data.stoi['_pad_']
        self.bs, self.stoi, self.itos = data.bs, data.stoi, {i: s for s, i in data.stoi.items()}
        self.enc = LSTM_Encoder(vocab_size, emb_dim, hidden_size, num_layers, pad_token, enc_drops, self.bs)
        if pretrained:
            raise NotImplementedError('wt103 pretrained weights are not part of the reference snapshot (LFS pointers)')
        self.dec = LanguageModelDecoder(vocab_size, emb_dim, dec_drop, tied_weight=self.enc.word_embed.embed.weight)
        self.head = self.dec
        self.layer_groups = [self.enc.lstms, self.head]
        self.param_groups = separate_bn_layers(self.layer_groups)

    def reset(self):
        self.enc.reset(self.bs)

    def clear_non_raw(self):
        self.to(default_device())
        for lstm in self.enc.lstms:
            lstm.clear_non_raw()

    def forward(self, x):
        return self.dec(self.enc(x))

    # ---- text generation (Text.py:655-676) -------------------------------------------------------------------------------------

    N_SPECIAL = 4          # the special tokens the reference never generates (`probs_next_token[:4] = 0`, Text.py:668)

    def predict_from_tokens(self, ids, n, k=5, seed=0, refeed=True, return_probs=False):
        """The next `n` token ids after the prompt `ids` (a list of token ids); returns the prompt plus the n new ids — the loop of
        the reference's predict_from_string (Text.py:660-676) on HIP kernels: eval(), enc.reset(bs=1) once, then per step softmax
        over the last position, entries [:4] (special tokens) zeroed, topk(k), one of the k drawn with probabilities
        top_probs / top_probs.sum(), appended; at the end enc.reset(bs=self.bs).  The model stays in eval mode.

        refeed=True (default) keeps the reference's quirk: EVERY iteration feeds the WHOLE sequence so far through the encoder with
        the hidden state carried over from the previous iteration.  refeed=False is the usual incremental decoder: the prompt goes
        through the encoder once, then each step feeds only the newest token through ops_text.lstm_cell_b1 (T = 1, B = 1).  Both end
        in ops_text.lm_next_token; the token buffer stays on the device and nothing is read back until all n steps are enqueued
        (one upload of prompt + uniforms, one copy back).

        Two deliberate differences from the reference: (1) the draw is SEEDED instead of coming from torch's global generator:
        step i uses u_i = float32(np.random.RandomState(seed).random_sample(n)[i]) and picks slot
        j = #{ m in 1..k-1 : c_m <= u_i * c_k }, c_m the sequential fp32 partial sums of the top probabilities in descending order;
        (2) tokenisation stays out of scope (as in TextDataset): this method takes ids, predict_from_string a `tokenize` callable.

        return_probs=True: also the per-step top_probs [n, k] (float32) and top_indices [n, k] (int64) as numpy arrays."""
        ids = [int(v) for v in ids]
        V = len(self.stoi)
        n, k = int(n), int(k)
        if len(ids) == 0:
            raise ValueError('predict_from_tokens: empty prompt')
        if n < 1:
            raise ValueError('predict_from_tokens: n must be at least 1')
        if k < 1 or k > 64:
            raise ValueError('predict_from_tokens: k must be in [1, 64]')
        if k > V - self.N_SPECIAL:
            raise ValueError('predict_from_tokens: k exceeds the %d tokens that are not special' % (V - self.N_SPECIAL))
        if min(ids) < 0 or max(ids) >= V:
            raise ValueError('predict_from_tokens: token id outside [0, %d)' % V)
        self.eval()
        self.enc.reset(1)
        dev = self.enc.word_embed.embed.weight.device
        L, nk = len(ids), n * k
        # ONE int64 buffer both ways: tokens [L + n] | uniforms (fp32 view) | top_indices [n, k] | top_probs (fp32 view)
        o_u = L + n
        o_idx = o_u + (n + 1) // 2
        o_p = o_idx + nk
        host = np.zeros(o_p + (nk + 1) // 2, dtype=np.int64)
        host[:L] = ids
        host[o_u:o_idx].view(np.float32)[:n] = np.random.RandomState(seed).random_sample(n).astype(np.float32)
        try:
            with torch.no_grad():
                buf = torch.from_numpy(host).to(dev)
                tokens, u = buf[:o_u], buf[o_u:o_idx].view(torch.float32)
                top_idx, top_p = buf[o_idx:o_p], buf[o_p:].view(torch.float32)
                self._generate_steps(tokens, u, top_p, top_idx, L, n, k, refeed)
                host = buf.cpu().numpy()
        finally:
            self.enc.reset(self.bs)
        out = [int(v) for v in host[:o_u]]
        if return_probs:
            return out, host[o_p:].view(np.float32)[:nk].reshape(n, k).copy(), host[o_idx:o_p].reshape(n, k).copy()
        return out

    def _generate_steps(self, tokens, u, top_p, top_idx, L, n, k, refeed):
        "enqueues the n steps of predict_from_tokens on device buffers; no host read (runs under torch.cuda.set_sync_debug_mode('error'))"
        emb = self.enc.word_embed.embed.weight.detach()
        V, E = emb.shape
        emb4 = ops_text.padded_rows(emb)                       # 16-byte rows for the decoder (emb itself when E % 4 == 0)
        pick = ops_text.LmNextToken(emb4, k, u, tokens, top_p, top_idx, self.N_SPECIAL, E)
        on = ops_text.stream()
        x = tokens.view(1, -1)

        def next_token(h, step):
            pick(h, step, L + step - 1, on)

        if refeed:
            for i in range(n):
                next_token(self.enc(x[:, :L + i])[-1, 0], i)
            return
        next_token(self.enc(x[:, :L])[-1, 0], 0)
        if n == 1:
            return
        # the padded weight copies, once per call; (h, c) of the prompt into zero-padded ping-pong buffers
        hbufs = []
        cells = [[], []]                                        # cells[q][l]: layer l reading its h buffer q, writing buffer 1 - q
        for l, lstm in enumerate(self.enc.lstms):
            p = lstm.lstm
            H = p.hidden_size
            hb = [torch.zeros((H + 3) // 4 * 4, dtype=torch.float32, device=emb.device) for _ in range(2)]
            hb[0][:H] = self.enc.h[l].reshape(-1)
            hbufs.append(hb)
            w_ih, w_hh = ops_text.padded_rows(p.weight_ih_l0), ops_text.padded_rows(p.weight_hh_l0_raw, w_hh=True)
            bias = (p.bias_ih_l0 + p.bias_hh_l0).detach().float().contiguous()
            c = self.enc.c[l].reshape(-1).float().clone()
            for q in (0, 1):                                    # every layer flips once per step: all read q, all write 1 - q
                below = hbufs[l - 1][1 - q] if l else None
                cells[q].append(ops_text.LstmCellB1(w_ih, w_hh, bias, hb[q], c, hb[1 - q], c, p.input_size, H, x=below,
                                                    emb=None if l else emb, tokens=None if l else tokens))
        for i in range(1, n):
            q = (i - 1) & 1
            for cell in cells[q]:
                cell(L + i - 1, on)
            next_token(hbufs[-1][1 - q], i)

    def predict_from_string(self, s, n, k=5, seed=0, refeed=True, tokenize=str.split):
        """The next n tokens after the string s, as a new string (Text.py:655-676).  `tokenize` (default str.split) stands in for the
        reference's spaCy tokeniser, which is not part of this package; tokens go through self.stoi, unknown ones to id 0 as
        numericalize does, then through predict_from_tokens (see there for k, seed, refeed and the two differences from the
        reference), and back through self.itos joined with spaces."""
        ids = [self.stoi.get(t, 0) for t in tokenize(s)]
        return ' '.join(self.itos[i] for i in self.predict_from_tokens(ids, n, k=k, seed=seed, refeed=refeed))


class TextClassificationNet(nn.Module):
    "LSTM_Encoder initialised from a language model + attention decoder (Text.py:704-751)"

    def __init__(self, PATH, language_model, num_classes, attn_size=100, enc_drops=[0.05, 0.25, 0.2, 0.15],
                 drop_scaling=0.7, fc_layer_sizes=[100], fc_drops=[0.25, 0.25]):
        super().__init__()
        import os
        enc_drops = list_mult(list(enc_drops), drop_scaling)
        lm_enc = language_model.enc
        emb_dim, hidden_size, num_layers = lm_enc.sizes[0], lm_enc.sizes[1], len(lm_enc.lstms)
        vocab_size, pad_token = len(language_model.stoi), language_model.stoi['_pad_']
        self.bs, self.stoi = language_model.bs, language_model.stoi
        PATH = correct_foldername(PATH)
        os.makedirs(PATH + 'models', exist_ok=True)
        torch.save(lm_enc.state_dict(), PATH + 'models/lang_model_enc.pt')
        self.enc = LSTM_Encoder(vocab_size, emb_dim, hidden_size, num_layers, pad_token, enc_drops, self.bs)
        self.enc.load_state_dict(torch.load(PATH + 'models/lang_model_enc.pt'), strict=False)
        self.dec = TextClassificationDecoder(emb_dim, num_classes, attn_size, fc_layer_sizes, fc_drops)
        self.head = self.dec
        self.layer_groups = [self.enc.lstms, self.enc.word_embed, self.head]
        self.param_groups = separate_bn_layers(self.layer_groups)

    def clear_non_raw(self):
        self.to(default_device())

    def forward(self, x, attn_vals=False):
        self.enc.reset(len(x))
        enc_out = self.enc(x)
        pred_classes, attn_values = self.dec(x, enc_out)
        return (pred_classes, enc_out, attn_values) if attn_vals else (pred_classes, enc_out)


# ---- losses / metrics (Text.py:756-808) --------------------------------------------------------------------------

class RegSeqCrossEntropyLoss(object):
    """CE(preds, target) + alpha*mean(enc_out^2) + beta*mean((enc_out[1:]-enc_out[:-1])^2) (Text.py:756-777).
    `.cross_entropy` keeps the unregularised CE as a detached 0-dim device tensor (the reference re-wraps
    loss.item(): same value, without the host sync)."""

    def __init__(self, alpha=2.0, beta=1.0):
        self.alpha, self.beta = alpha, beta
        self.cross_entropy = torch.zeros(())

    def __call__(self, outputs, target):
        preds, enc_out = outputs
        loss = ops.cross_entropy_nd(preds, target)
        self.cross_entropy = loss.detach()
        if enc_out.is_cuda and enc_out.dim() == 3 and (self.alpha > 0 or self.beta > 0):
            # alpha * mean(h^2) + beta * mean((h[1:] - h[:-1])^2) in one reduction kernel (ops_text.seq_activation_reg)
            return loss + ops.seq_activation_reg(enc_out, max(self.alpha, 0.0), max(self.beta, 0.0))
        if self.alpha > 0:
            loss = loss + self.alpha * enc_out.pow(2).mean()
        if self.beta > 0:
            loss = loss + self.beta * (enc_out[1:] - enc_out[:-1]).pow(2).mean()
        return loss


class SeqCrossEntropyLoss(object):
    "The unregularised CE of a RegSeqCrossEntropyLoss instance (Text.py:779-788)"
    def __init__(self, regularized_loss):
        self.regularized_loss = regularized_loss

    def __call__(self, outputs, target):
        return self.regularized_loss.cross_entropy


class LanguageModelAccuracy(object):
    "Next-token accuracy ignoring the 4 special tokens (Text.py:791-799)"
    def __call__(self, outputs, target):
        preds, _ = outputs
        preds[:, :4, :] = 0
        return (preds.max(dim=1)[1] == target).sum().float() / (target.shape[0] * target.shape[1])


class TextClassificationAccuracy(object):
    "Text.py:801-808"
    def __call__(self, outputs, target):
        preds, _ = outputs
        return (preds.max(dim=1)[1] == target).sum().float() / len(target)
