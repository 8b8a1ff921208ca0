"""Golden G26 for the text data side (reference Applications/Text.py:28-122: Tokenizer's host rules, do_caps, numericalize).

Runs the REAL reference on CPU through oracle/_ref_import.py (read-only) and writes data only, to tests/golden/g26_text_tokens.json.
Nothing here needs a spaCy instance: Tokenizer.re_rep, re_word_rep, replace_rep, replace_wrep and do_caps are class attributes and
static methods, and numericalize is pure Python (its prints are swallowed).

  texts        40 short ASCII texts: contractions, all-capitals words, digits with '.' and ',', repeated punctuation, <br />, the
               special tokens, repeated characters and repeated words.  None has an all-capitals run that begins inside a token
               (O'CLOCK, 3.5AB): there do_caps' inserted spaces split the token, a documented difference of the package's grammar.
  rep          texts after re_rep.sub(replace_rep)
  wrep         `rep` after re_word_rep.sub(replace_wrep)
  caps         do_caps(text) of every raw text
  num_ss       6 lists of token strings with planted count ties (a / b 9 times, c / d 7, e / f 6), tokens below the default min_freq
               and one token that is spelled like a special (_pad_)
  num_cases    for (max_vocab, min_freq) in (60000, 6), (5, 2) — the cut bites before min_freq: f occurs 6 times and is cut — and
               (6, 7): numericalize's ids and its stoi as an ordered list of [token, id]
  num_given    the same token lists through numericalize with the stoi of the (5, 2) case, which lacks f, g, h, ...: the ids
Usage: python tools/gen_golden_text_tokens.py   (needs the reference checkout the oracle shim points at)"""
import contextlib
import io
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g26_text_tokens.json')

TEXTS = [
    "DON'T do that",
    "it's 3.5/10!!!",
    "I loved it<br />SO MUCH, really",
    "Sooooo good",
    "yes yes yes yes yes indeed",
    "<eos> marks the end and <bos> the start",
    "an <unk> word",
    "o'clock already",
    "NASA's rocket",
    "WALL-E was GREAT",
    "U.S.A. and U.K.",
    "AT&T or IBM",
    "ABC1.5 is a version",
    "1,000 dollars -- cheap",
    "wait... what?!",
    "He said: \"no way\"",
    "they're here, we'll go",
    "couldn't've done it",
    "I CAN'T EVEN",
    "n't",
    "",
    "   ",
    "x",
    "a/b #tag",
    "!!!!!! wow",
    "line one\nline two\ttabbed",
    "end without space.",
    "MIXED Case Words HERE",
    "snake_case and CONST_NAME",
    "rock'n'roll",
    "'quoted' text",
    "e-mail me @ home",
    "100% sure",
    "so so so so so so tired",
    "A+ movie",
    "(parenthetical) [bracketed] {braced}",
    "semi;colon and co:lon",
    "7 out of 10",
    "The END",
    "ok<br>fine<BR/>done",
]


def token_lists():
    counts = [('a', 9), ('b', 9), ('c', 7), ('d', 7), ('e', 6), ('f', 6), ('g', 5), ('h', 3), ('i', 2), ('j', 1), ('_pad_', 8), ("n't", 4),
              ('t_up', 4), ('3.5', 2)]
    bag = [t for t, c in counts for _ in range(c)]
    random.Random(26).shuffle(bag)
    cuts = [0, 11, 12, 30, 30, 52, len(bag)]          # one list of a single token, one empty list
    return [bag[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]


def main():
    from oracle import _ref_import
    TX = _ref_import.load()['Applications.Text']
    T = TX.Tokenizer
    rep = [T.re_rep.sub(T.replace_rep, s) for s in TEXTS]
    wrep = [T.re_word_rep.sub(T.replace_wrep, s) for s in rep]
    caps = [T.do_caps(s) for s in TEXTS]
    ss = token_lists()

    def numericalize(**kw):
        with contextlib.redirect_stdout(io.StringIO()):
            ids, stoi = TX.numericalize([list(s) for s in ss], **kw)
        return ids, stoi

    cases = []
    for max_vocab, min_freq in ((60000, 6), (5, 2), (6, 7)):
        ids, stoi = numericalize(max_vocab=max_vocab, min_freq=min_freq)
        cases.append({'max_vocab': max_vocab, 'min_freq': min_freq, 'ids': ids, 'stoi': [[k, v] for k, v in stoi.items()]})
    given = dict(cases[1]['stoi'])
    ids, stoi = numericalize(stoi=given)
    assert stoi == given
    out = {'texts': TEXTS, 'rep': rep, 'wrep': wrep, 'caps': caps, 'num_ss': ss, 'num_cases': cases, 'num_given': {'case': 1, 'ids': ids}}
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
