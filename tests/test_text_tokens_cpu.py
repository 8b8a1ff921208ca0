"""Text data side (K17), without a GPU: the tests' restatement of the grammar against hand-written token lists and against golden G26
(the reference's host rules, do_caps and numericalize), the package's host pre-rules against G26, the grammar functions the kernels
compile (csrc/text_grammar.h) run on the host against the restatement, and the argument checks of the nnl_text_* entries."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import text_tokens_restatement as R
from conftest import ROOT

CASES = [
    ("DON'T", ['t_up', 'do', "n't"]),
    ("it's 3.5/10!!!", ['it', "'s", '3.5', '/', '10', '!!!']),
    ('<eos>', ['<eos>']),
    ('a<unk>b <bos>', ['a', '<unk>', 'b', '<bos>']),
    ('<<unk>>', ['<', '<unk>', '>']),
    ('<EOS>', ['<', 't_up', 'eos', '>']),
    ("n't", ["n't"]),
    ("o'clock", ['o', "'clock"]),
    ("O'CLOCK", ['o', "'clock"]),                     # the run CLOCK begins inside a token: no t_up (a documented difference)
    ('--', ['--']),
    ('a--b...c', ['a', '--', 'b', '...', 'c']),
    ('-!-', ['-', '!', '-']),
    ('naïve café', ['naïve', 'café']),
    ('ÉCOLE É', ['t_up', 'École', 'É']),      # non-ASCII letters are never cased, but count as bytes of the run
    ('', []),
    (' \t\n\r\x0b\x0c ', []),
    ('1,000 and 3.5. x,y 1.', ['1,000', 'and', '3.5', '.', 'x', ',', 'y', '1', '.']),
    ("couldn't've", ['could', "n't", "'ve"]),
    ("rock'n'roll", ['rock', "'n", "'roll"]),
    ("'quoted'", ["'", 'quoted', "'"]),
    ('NASA AT IBM_1', ['t_up', 'nasa', 'at', 't_up', 'ibm_1']),
    ('ABC1.5', ['t_up', 'abc1.5']),
    ('t_up T_UP', ['t_up', 't_up', 't_up']),
    ("isn't", ['is', "n't"]),
    ("ain'tx", ['ain', "'tx"]),
]


@pytest.mark.parametrize('text,want', CASES, ids=[repr(c[0]) for c in CASES])
def test_restatement_gives_the_hand_written_tokens(text, want):
    assert R.tokens(text) == want


def test_restatement_split_mode_is_str_split_on_ascii_whitespace():
    assert R.tokens("  DON'T  stop\tme<eos>\n", R.SPLIT_MODE) == ["DON'T", 'stop', 'me<eos>']
    assert R.tokens('', R.SPLIT_MODE) == [] and R.tokens(' \n', R.SPLIT_MODE) == []


def test_package_pre_rules_equal_g26():
    from neuralnetworklibrary_amd.Applications.Text import Tokenizer
    g = R.g26()
    tok = Tokenizer()
    assert len(g['texts']) == 40 and all(t.isascii() for t in g['texts'])
    rep = [Tokenizer.re_rep.sub(Tokenizer.replace_rep, s) for s in g['texts']]
    assert rep == g['rep']
    wrep = [Tokenizer.re_word_rep.sub(Tokenizer.replace_wrep, s) for s in rep]
    assert wrep == g['wrep']
    assert any(a != b for a, b in zip(g['texts'], g['rep'])) and any(a != b for a, b in zip(g['rep'], g['wrep']))
    for s, w in zip(g['texts'], wrep):
        assert tok.pre_rules(s) == R.pre_rules(s) == R.PRE[3][0].sub(R.PRE[3][1], R.PRE[2][0].sub(R.PRE[2][1], w))
    assert tok.sub_br('a<br />b<BR>c< br/>d') == 'a\nb\nc\nd'


def test_case_rule_is_the_reference_do_caps_on_ascii():
    "the grammar on do_caps' output (lowered text with ' t_up ' written in) gives the tokens the grammar's own case rule gives on the raw text"
    g = R.g26()
    n_up = 0
    for raw, caps in zip(g['texts'], g['caps']):
        assert R.tokens(caps) == R.tokens(raw), raw
        n_up += R.tokens(raw).count('t_up')
    assert n_up >= 10


def test_restatement_numericalize_equals_g26():
    g = R.g26()
    ss = g['num_ss']
    assert any(len(s) == 0 for s in ss)
    for case in g['num_cases']:
        ids, stoi = R.numericalize(ss, case['max_vocab'], case['min_freq'])
        assert ids == case['ids'] and [[k, v] for k, v in stoi.items()] == case['stoi']
    given = dict(g['num_cases'][g['num_given']['case']]['stoi'])
    ids, stoi = R.numericalize(ss, stoi=given)
    assert ids == g['num_given']['ids'] and stoi == given and any(0 in s for s in ids)


# ---- the grammar functions the kernels compile, on the host ------------------------------------------------------------------------

def _compiler():
    for name in ('c++', 'g++', 'clang++'):
        if shutil.which(name):
            return name
    raise AssertionError('no C++ compiler on PATH to build tools/text_grammar_check.cpp')


def test_kernel_grammar_functions_equal_the_restatement_on_the_host(tmp_path):
    """csrc/text_grammar.h (starts_at, token_length: what every kernel thread evaluates for its byte) through
    tools/text_grammar_check.cpp: the hand-written cases, G26's texts and 4 000 seeded random texts over an alphabet of the bytes the
    rules look at, laid end to end with NO separator, both modes."""
    exe = str(tmp_path / 'text_grammar_check')
    subprocess.run([_compiler(), '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'text_grammar_check.cpp'), '-o', exe], check=True)
    rng = random.Random(17)
    alpha = ['a', 'n', 'N', 't', 'T', "'", '.', ',', '1', '5', '<', '>', 'eos', 'unk', 'bos', '<unk>', '<eos>', 'A', 'B', 'C', '-', '!',
             '_', 'é', '\n', ' ', ' ', "n't", "N'T", "'s"]
    texts = [c[0] for c in CASES] + R.g26()['texts'] + [''.join(rng.choice(alpha) for _ in range(rng.randint(0, 12))) for _ in range(4000)]
    texts = [t.encode('utf-8') for t in texts]
    off = [0]
    for t in texts:
        off.append(off[-1] + len(t))
    (tmp_path / 'bytes.bin').write_bytes(b''.join(texts))
    (tmp_path / 'off.txt').write_text(' '.join(map(str, off)))
    for mode in (R.GRAMMAR_MODE, R.SPLIT_MODE):
        out = subprocess.run([exe, str(mode), str(tmp_path / 'bytes.bin'), str(tmp_path / 'off.txt')], capture_output=True, text=True, check=True)
        got = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
        want = [(s + off[j], l) for j, t in enumerate(texts) for s, l in R.records(t, mode)]
        assert got == want, 'mode %d' % mode


# ---- the C entries: arguments are checked before any HIP call ---------------------------------------------------------------------------

def _entries():
    """name -> (argument list builder, the keys it honours).  p is a non-null pointer that is never dereferenced: every call the test
    makes fails its argument check, so nothing is launched."""
    p, one, cap = C.c_void_p(8), 1, 1024
    g = lambda k, name, dflt: k.get(name, dflt)
    return {
        'nnl_text_token_count': (lambda k: [g(k, 'ptr', p), g(k, 'B', one), p, g(k, 'n', one), g(k, 'mode', 0), p, None], 'ptr B n mode'),
        'nnl_text_token_fill': (lambda k: [g(k, 'ptr', p), g(k, 'B', one), p, g(k, 'n', one), g(k, 'mode', 0), p, g(k, 'T', one), p, p, p, None],
                                'ptr B n mode T'),
        'nnl_text_token_hash': (lambda k: [g(k, 'ptr', p), g(k, 'B', one), p, p, g(k, 'T', one), g(k, 'mode', 0), 0, g(k, 'mask', 1), p, None],
                                'ptr B T mode mask'),
        'nnl_text_vocab_insert': (lambda k: [g(k, 'ptr', p), g(k, 'T', one), p, p, p, g(k, 'cap', cap), 1, p, p, None], 'ptr T cap'),
        'nnl_text_vocab_verify': (lambda k: [g(k, 'ptr', p), g(k, 'B', one), p, p, p, g(k, 'T', one), g(k, 'mode', 0), p, one, p, p, one, 0, p,
                                             g(k, 'cap', cap), p, None], 'ptr B T mode cap'),
        'nnl_text_vocab_compact': (lambda k: [g(k, 'ptr', p), p, p, g(k, 'cap', cap), p, p, g(k, 'T', one), p, one, p, None], 'ptr cap T'),
        'nnl_text_vocab_assign': (lambda k: [g(k, 'ptr', p), p, g(k, 'T', one), p, g(k, 'cap', cap), None], 'ptr T cap'),
        'nnl_text_vocab_lookup': (lambda k: [g(k, 'ptr', p), g(k, 'B', one), p, p, p, g(k, 'T', one), g(k, 'mode', 0), p, one, p, p, one, p, p,
                                             g(k, 'cap', cap), p, None], 'ptr B T mode cap'),
        'nnl_text_ids_write': (lambda k: [g(k, 'ptr', p), p, g(k, 'cap', cap), p, g(k, 'n', one), g(k, 'T', one), 0, p, None], 'ptr cap n T'),
    }


BAD = {'ptr': [(None, b'null')], 'T': [(-1, b'')], 'B': [(-1, b''), (2 ** 31, b'')], 'n': [(0, b''), (-3, b'')], 'mode': [(2, b'mode')],
       'cap': [(1000, b'power of two'), (-16, b'power of two'), (8, b'power of two')], 'mask': [(0, b'hash_mask')]}


@pytest.mark.parametrize('name', sorted(_entries()))
def test_text_entries_reject_null_and_negative_arguments(name):
    from neuralnetworklibrary_amd._lib import lib
    build, keys = _entries()[name]
    for key in keys.split():
        for value, word in BAD[key]:
            assert getattr(lib, name)(*build({key: value})) == -1, (key, value)
            err = lib.nnl_last_error()
            assert name[4:].encode() in err and word in err, (key, value, err)


def test_text_constants_match_the_header():
    import re
    from neuralnetworklibrary_amd import ops_text
    header = open(os.path.join(ROOT, 'include', 'nnl.h')).read()
    assert int(re.search(r'#define\s+NNL_TEXT_TILE\s+(\d+)', header).group(1)) == ops_text.TEXT_TILE
    assert int(re.search(r'#define\s+NNL_TEXT_TUP_LEN\s+\((-?\d+)\)', header).group(1)) == ops_text.TEXT_TUP_LEN == R.TUP
    assert 'NNL_TEXT_MODE_GRAMMAR = 0, NNL_TEXT_MODE_SPLIT = 1' in header and 'NNL_TEXT_STATUS_OVERFLOW = 1' in header
    assert (ops_text.TEXT_MODE_GRAMMAR, ops_text.TEXT_MODE_SPLIT, ops_text.TEXT_STATUS_OVERFLOW) == (0, 1, 1)
    assert ops_text.vocab_capacity(0) == 1024 and ops_text.vocab_capacity(513) == 2048 and ops_text.vocab_capacity(5000) == 16384


# ---- Python API without a GPU ----------------------------------------------------------------------------------------------------

def test_the_five_calls_without_a_tokenizer_still_raise():
    from neuralnetworklibrary_amd.Applications.Text import LanguageModelDataObj, TextClassificationDataObj, TextDataset
    with pytest.raises(NotImplementedError):
        TextDataset(['a raw string needs a tokenizer'], [0])
    with pytest.raises(NotImplementedError):
        TextDataset.from_csv('train.csv', 'text', 'label')
    with pytest.raises(NotImplementedError):
        TextDataset.from_text_files('train', ['neg', 'pos'])
    with pytest.raises(NotImplementedError):
        TextClassificationDataObj.from_csv(16, 'train.csv')
    with pytest.raises(NotImplementedError):
        TextClassificationDataObj.from_folders(16, ['neg', 'pos'], 'train')
    with pytest.raises(NotImplementedError):
        LanguageModelDataObj.from_csv(16, 70, 'train.csv')
    with pytest.raises(NotImplementedError):
        LanguageModelDataObj.from_folders(16, 70, None, 'train')
    ds = TextDataset([[5, 6, 7], [8]], ['b', 'a'], stoi={'_pad_': 1}, reverse=True)            # id lists: unchanged
    assert list(ds.texts) == [[7, 6, 5], [8]] and ds.num_tokens == 4 and list(ds.labels) == [1, 0]


def test_numericalize_and_corpus_refuse_what_they_cannot_represent():
    from neuralnetworklibrary_amd import ops_text
    from neuralnetworklibrary_amd.Applications.Text import numericalize
    for bad in ('two words', '', 'tab\there', 'nl\n'):
        with pytest.raises(ValueError):
            numericalize([['fine', bad]])
    with pytest.raises(ValueError):
        ops_text.TextCorpus(b'abc', [0, 2])              # offsets must end at len(data)
    with pytest.raises(ValueError):
        ops_text.TextCorpus(b'abc', [0, 2, 1, 3])        # and never decrease
    with pytest.raises(ValueError):
        ops_text.TextCorpus.from_texts([])
