"""The yardstick of tests/test_text_tokens_cpu.py and tests/test_text_tokens_gpu.py: the text grammar of DESIGN.md section 8 restated as ONE
`re` pattern plus the case rule, and numericalize restated with Counter / most_common / defaultdict (reference Applications/Text.py:95-122).
Nothing here imports the package."""
import collections
import json
import os
import re

from conftest import GOLDEN

RAW = rb'[0-9A-Za-z_\x80-\xff]'                                   # a W byte proper
WB = rb'(?:' + RAW + rb'|(?<=[0-9])[.,](?=[0-9]))'                # W with the digit rule
SPECIAL = rb'<(?:eos|bos|unk)>'
NT = rb"[nN]'[tT](?!" + RAW + rb')'                               # n't, the run after the apostrophe exactly t / T
WORD = rb'(?:(?!' + NT + rb')' + WB + rb')'                       # a word byte at which no n't begins
GRAMMAR = re.compile(rb'|'.join([
    SPECIAL,
    NT,
    rb'(?<=' + RAW + rb")'(?=" + RAW + rb')' + WORD + rb'*',       # 's 're 'll
    WORD + rb'+',
    rb'(?!' + SPECIAL + rb')([^\s0-9A-Za-z_\x80-\xff])(?:(?!' + SPECIAL + rb')\1)*',      # one repeated P byte
]))
RUN = re.compile(RAW + rb'+')
TUP = -1
GRAMMAR_MODE, SPLIT_MODE = 0, 1


def records(text, mode=GRAMMAR_MODE):
    "[(start, len)] of one text's tokens (bytes), len TUP for the pseudo-token t_up"
    if mode == SPLIT_MODE:
        return [(m.start(), len(m.group())) for m in re.finditer(rb'\S+', text)]
    out = []
    for m in GRAMMAR.finditer(text):
        s = m.start()
        run = RUN.match(text, s)
        if run and (s == 0 or not RUN.match(text, s - 1)):       # a run of W bytes proper begins with this token
            r = run.group()
            if len(r) > 2 and re.search(rb'[A-Z]', r) and not re.search(rb'[a-z]', r):
                out.append((s, TUP))
        out.append((s, len(m.group())))
    return out


def tokens(text, mode=GRAMMAR_MODE):
    "token strings of one text (str or bytes)"
    b = text.encode('utf-8') if isinstance(text, str) else text
    out = []
    for s, l in records(b, mode):
        t = b't_up' if l == TUP else b[s:s + l]
        out.append((t.lower() if mode == GRAMMAR_MODE else t).decode('utf-8'))
    return out


PRE = [(re.compile(r'(\S)(\1{3,})'), lambda m: ' tk_rep %d %s ' % (len(m.group(2)) + 1, m.group(1))),
       (re.compile(r'(\b\w+\W+)(\1{3,})'), lambda m: ' tk_wrep %d %s ' % (len(m.group(2).split()) + 1, m.group(1))),
       (re.compile(r'<\s*br\s*/?>', re.IGNORECASE), '\n'),
       (re.compile(r'([/#])'), r' \1 ')]


def pre_rules(s):
    for pat, rep in PRE:
        s = pat.sub(rep, s)
    return s


def numericalize(ss, max_vocab=60000, min_freq=6, stoi=None):
    if stoi is None:
        common = collections.Counter(t for s in ss for t in s).most_common(max_vocab)
        names = ['_unk_', '_pad_', '_bos_', '_eos_'] + [t for t, c in common if c >= min_freq]
        stoi = {t: i for i, t in enumerate(names)}
    look = collections.defaultdict(lambda: 0, stoi)
    return [[look[t] for t in s] for s in ss], stoi


def chain(texts, max_vocab=60000, min_freq=6, stoi=None, reverse=False):
    "what TextDataset(strings, tokenizer=...) must equal: pre-rules, grammar, numericalize, reversal"
    ids, stoi = numericalize([tokens(pre_rules(t)) for t in texts], max_vocab, min_freq, stoi)
    return ([list(reversed(t)) for t in ids] if reverse else ids), stoi


def g26():
    with open(os.path.join(GOLDEN, 'g26_text_tokens.json')) as f:
        return json.load(f)
