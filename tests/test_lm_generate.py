"""Text generation (K5d): LanguageModelNet.predict_from_tokens / predict_from_string (reference Applications/Text.py:655-676) on
nnl_lstm_cell_b1 and nnl_lm_next_token.

CPU: an fp64 restatement (pure torch: LSTM cell, softmax, special-token mask, top-k, the seeded draw rule) of the reference's loop
(refeed=True) and of the incremental loop (refeed=False), pinned to the golden G20 that tools/gen_golden_lm_generate.py recorded
from the real reference; string mapping and argument errors.  GPU: each C entry and both loops against that restatement.

Tolerances are measured, not chosen: the same computation is run on the CPU in fp32 and its distance d from fp64 is the yardstick
(10 d for values).  d is floored at 2^-24 times the largest reference value: no fp32 result can be asked to come closer than half
a unit in the last place.  Where an index or a token must be EQUAL, the inputs are drawn until the restatement's three margins (the
gap between the k-th and the (k+1)-th eligible logit, the distance of u c_k from every c_m, the gap between adjacent top
probabilities) exceed 100 d; 50 draws without one is a failure, never a skip."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_close, load_golden
from oracle import reference_text as RT
from oracle import synth

DEV = 'cuda'
N_SPECIAL = 4
F32_HALF_ULP = 2.0 ** -24


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def cell(x, h, c, w_ih, w_hh, b):
    "one LSTM cell on vectors, torch's gate order i, f, g, o; b = b_ih + b_hh"
    g = w_ih @ x + w_hh @ h + b
    H = h.numel()
    c2 = torch.sigmoid(g[H:2 * H]) * c + torch.sigmoid(g[:H]) * torch.tanh(g[2 * H:3 * H])
    return torch.sigmoid(g[3 * H:]) * torch.tanh(c2), c2


def draw_slot(top_probs, u):
    "slot j = #{ m in 1..k-1 : c_m <= u c_k }, c_m the sequential partial sums in top_probs' own precision; also min |u c_k - c_m|"
    c, cs = top_probs.new_zeros(()), []
    for p in top_probs:
        c = c + p
        cs.append(c)
    t = torch.as_tensor(float(u), dtype=top_probs.dtype) * cs[-1]
    return sum(1 for cm in cs[:-1] if bool(cm <= t)), min([abs(float(cm) - float(t)) for cm in cs[:-1]] or [float('inf')])


def next_token(emb, h, k, u):
    "(token, top_probs [k], top_indices [k], smallest of the three margins) of Text.py:667-672 with the seeded draw"
    logits = emb @ h
    p = torch.softmax(logits, dim=0)
    p[:N_SPECIAL] = 0
    tp, ti = torch.topk(p, k)
    j, m_draw = draw_slot(tp, u)
    elig = logits[N_SPECIAL:].double().sort(descending=True)[0]
    m_logit = float(elig[k - 1] - elig[k]) if k < elig.numel() else float('inf')
    m_adj = min([float(tp[m] - tp[m + 1]) for m in range(k - 1)] or [float('inf')])
    return int(ti[j]), tp, ti, min(m_logit, m_draw, m_adj)


def lm_params(net, dtype=torch.float64):
    "{'emb': [V, E], 'layers': [(w_ih, w_hh, b_ih + b_hh)]} of a LanguageModelNet (product, oracle or reference naming alike), on the CPU"
    sd = {k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()}
    layers, l = [], 0
    while 'enc.lstms.%d.lstm.weight_ih_l0' % l in sd:
        pre = 'enc.lstms.%d.lstm.' % l
        layers.append((sd[pre + 'weight_ih_l0'], sd[pre + 'weight_hh_l0_raw'], sd[pre + 'bias_ih_l0'] + sd[pre + 'bias_hh_l0']))
        l += 1
    return {'emb': sd['enc.word_embed.embed.weight'], 'layers': layers}


def generate(P, prompt, n, k, u, refeed):
    """the reference's loop (refeed=True: every iteration feeds the WHOLE sequence so far, the state carried from the previous
    iteration) or the incremental one (refeed=False) in P's precision -> tokens, top_probs [n, k], top_indices [n, k], margin"""
    dt = P['emb'].dtype
    state = [(torch.zeros(w_hh.shape[1], dtype=dt), torch.zeros(w_hh.shape[1], dtype=dt)) for _, w_hh, _ in P['layers']]
    toks, probs, idxs, margin = list(prompt), [], [], float('inf')

    def feed(ids):
        for t in ids:
            x = P['emb'][t]
            for l, (w_ih, w_hh, b) in enumerate(P['layers']):
                state[l] = cell(x, state[l][0], state[l][1], w_ih, w_hh, b)
                x = state[l][0]
        return x

    for i in range(n):
        top = feed(toks if (refeed or i == 0) else toks[-1:])
        tok, tp, ti, m = next_token(P['emb'], top, k, u[i])
        toks.append(tok); probs.append(tp); idxs.append(ti); margin = min(margin, m)
    return toks, torch.stack(probs), torch.stack(idxs), margin


def uniforms(seed, n):
    return np.random.RandomState(seed).random_sample(n).astype(np.float32)


def distance(a32, a64):
    "fp32-vs-fp64 distance of one CPU computation, floored at half a unit in the last place of the largest value"
    a64 = a64.double()
    return max(float((a32.double() - a64).abs().max()), F32_HALF_ULP * float(a64.abs().max()))


def to32(P):
    return {'emb': P['emb'].float(), 'layers': [tuple(t.float() for t in lay) for lay in P['layers']]}


def seeds_with_margin(P, prompt, n, k, refeed, want=1):
    """the first `want` seeds (of 50) at which the fp64 restatement's margins exceed 100 x the fp32-fp64 distance of its probabilities;
    each as (seed, tokens, probs, idx, d).  Fewer than `want` is a failure."""
    P32, found = to32(P), []
    for seed in range(50):
        u = uniforms(seed, n)
        t64, p64, i64, margin = generate(P, prompt, n, k, u, refeed)
        t32, p32, i32, _ = generate(P32, prompt, n, k, u, refeed)
        d = distance(p32, p64) if t32 == t64 and torch.equal(i32, i64) else float('inf')
        if margin > 100 * d:
            found.append((seed, t64, p64, i64, d))
            if len(found) == want:
                return found
    raise AssertionError('50 seeds gave %d of %d cases whose margins exceed 100 x the fp32-fp64 distance' % (len(found), want))


# ---- nets --------------------------------------------------------------------------------------------------------------------------

def vocab(V, bs=3):
    from neuralnetworklibrary_amd.Applications.Text import _Vocab
    stoi = {'w%d' % i: i for i in range(V)}
    stoi['_pad_'] = 1
    del stoi['w1']
    return _Vocab(stoi, bs)


def product_net(V, tag, scale, device, **sizes):
    from neuralnetworklibrary_amd.Applications.Text import LanguageModelNet
    net = LanguageModelNet(vocab(V), **sizes)
    synth.fill_lm_reference_init_(net, seed=tag)
    with torch.no_grad():
        net.enc.word_embed.embed.weight.mul_(scale)
    return net.to(device)


@pytest.fixture(scope='module')
def g20():
    return load_golden('g20_lm_generate')


@pytest.fixture(scope='module')
def g20_net(g20):
    "the product net of G20 (400 / 1150 / 3, V = 61) on the GPU and its fp64 parameters"
    net = product_net(int(g20['V']), int(g20['tag']), float(g20['scale']), DEV)
    return net, lm_params(net)


@pytest.fixture(scope='module')
def small_net():
    net = product_net(61, 3, 60.0, DEV, emb_dim=12, hidden_size=37, num_layers=2)
    return net, lm_params(net)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_restatement_reproduces_g20(g20):
    "the fp64 restatement of the reference's loop gives G20's tokens exactly and its fp64 probabilities within the stored distance"
    net = RT.LanguageModelNet(int(g20['V']), 1, 1)
    synth.fill_lm_reference_init_(net, seed=int(g20['tag']))
    P = lm_params(net)
    P['emb'] = P['emb'] * float(g20['scale'])
    assert np.array_equal(g20['u'], uniforms(int(g20['seed']), int(g20['n'])))
    assert float(g20['margin']) >= 100 * float(g20['d'])
    for k in (5, 1):
        toks, probs, idxs, _ = generate(P, [int(t) for t in g20['prompt']], int(g20['n']), k, g20['u'], refeed=True)
        assert toks == [int(t) for t in g20['tokens.k%d' % k]]
        assert np.array_equal(idxs.numpy(), g20['top_indices.k%d' % k])
        assert float(np.abs(probs.numpy() - g20['top_probs.k%d.f64' % k]).max()) <= float(g20['d'])
        assert float(np.abs(g20['top_probs.k%d.f32' % k] - g20['top_probs.k%d.f64' % k]).max()) <= float(g20['d'])


def test_predict_from_string_maps_unknown_words_to_0_and_round_trips(monkeypatch):
    net = product_net(61, 0, 1.0, 'cpu', emb_dim=12, hidden_size=37, num_layers=2)
    seen = {}

    def fake(ids, n, k=5, seed=0, refeed=True, return_probs=False):
        seen.update(ids=list(ids), n=n, k=k, seed=seed, refeed=refeed)
        return list(ids) + [9, 4]
    monkeypatch.setattr(net, 'predict_from_tokens', fake)
    net.itos[0] = '_unk_'
    out = net.predict_from_string('w7 nosuchword w23 _pad_', 2, k=3, seed=11, refeed=False)
    assert seen == {'ids': [7, 0, 23, 1], 'n': 2, 'k': 3, 'seed': 11, 'refeed': False}
    assert out == 'w7 _unk_ w23 _pad_ w9 w4'
    assert net.predict_from_string('w7,w5', 2, tokenize=lambda s: s.split(',')) == 'w7 w5 w9 w4'


@pytest.mark.parametrize('ids,n,k', [([], 3, 5), ([5, 6], 0, 5), ([5, 6], 3, 0), ([5, 6], 3, 65), ([5, 6], 3, 58)])
def test_argument_errors_raise_value_error(ids, n, k):
    "an empty prompt, n < 1, k < 1, k > 64, k > V - 4 (V = 61: 57 eligible tokens)"
    net = product_net(61, 0, 1.0, 'cpu', emb_dim=12, hidden_size=37, num_layers=2)
    with pytest.raises(ValueError):
        net.predict_from_tokens(ids, n, k=k)
    assert net.enc.h[0].shape[1] == net.bs


# ---- GPU: nnl_lstm_cell_b1 ---------------------------------------------------------------------------------------------------------

def _ceil4(n):
    return (n + 3) // 4 * 4


def _cell_case(I, H):
    g = torch.Generator().manual_seed(1000 * I + H)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    k = 1.0 / H ** 0.5
    return {'w_ih': r(4 * H, I) * k, 'w_hh': r(4 * H, H) * k, 'b': r(4 * H) * 2 * k, 'x': r(I), 'h': r(H) * 0.5, 'c': r(H),
            'table': r(7, I)}


@pytest.mark.gpu
@pytest.mark.parametrize('token_input', [False, True])
@pytest.mark.parametrize('I,H', [(13, 37), (64, 64), (400, 1150), (1150, 1150), (1150, 400)])
def test_lstm_cell_b1_vs_fp64(I, H, token_input):
    """one cell against fp64, within 10 x the distance of the same cell in torch CPU fp32 (recomputed here); c_out aliases c; two calls
    on the same inputs are bitwise equal.  token_input: the input is the LAST row of a 7-row table, its id read on the device."""
    from neuralnetworklibrary_amd import ops_text
    q = _cell_case(I, H)
    if token_input:
        q['table'][6] = q['x']
    h64, c64 = cell(q['x'], q['h'], q['c'], q['w_ih'], q['w_hh'], q['b'])
    h32, c32 = cell(*(q[n].float() for n in ('x', 'h', 'c', 'w_ih', 'w_hh', 'b')))
    d_h, d_c = distance(h32, h64), distance(c32, c64)
    dev = lambda t: t.float().to(DEV)
    w_ih, w_hh = ops_text.padded_rows(dev(q['w_ih'])), ops_text.padded_rows(dev(q['w_hh']), w_hh=True)
    assert w_ih.shape[1] == _ceil4(I) and w_hh.shape[1] == _ceil4(H)
    pad = lambda v, n: torch.nn.functional.pad(dev(v), (0, n - v.numel()))
    h, x = pad(q['h'], _ceil4(H)), None if token_input else pad(q['x'], _ceil4(I))
    table = dev(q['table']) if token_input else None
    tokens = torch.tensor([3, 0, 6, 2], device=DEV) if token_input else None
    outs = []
    for _ in range(2):
        h_out, c = torch.zeros(_ceil4(H), device=DEV), dev(q['c'])
        ops_text.lstm_cell_b1(w_ih, w_hh, dev(q['b']), h, c, h_out, c, I, H, x=x, emb=table, tokens=tokens, pos=2)
        outs.append((h_out.cpu(), c.cpu()))
    print('cell (%d, %d): |hip - f64| h %.2e c %.2e; torch fp32 h %.2e c %.2e' % (
        I, H, float((outs[0][0][:H].double() - h64).abs().max()), float((outs[0][1].double() - c64).abs().max()), d_h, d_c))
    assert float((outs[0][0][:H].double() - h64).abs().max()) <= 10 * d_h
    assert float((outs[0][1].double() - c64).abs().max()) <= 10 * d_c
    assert float(outs[0][0][H:].abs().sum()) == 0.0, 'the pad entries of h_out are never written'
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
def test_lstm_cell_b1_refuses_unpadded_rows_and_launches_nothing():
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    I, H = 13, 37
    z = lambda *s: torch.zeros(*s, device=DEV)
    w_ih, w_hh, b, x, h, c = z(4 * H, 16), z(4 * H, 40), z(4 * H), z(16), z(40), z(H)
    h_out, c_out = torch.full((40,), 7.0, device=DEV), torch.full((H,), 7.0, device=DEV)
    call = lambda ldi, ldh, ho: lib.nnl_lstm_cell_b1(ptr(w_ih), ldi, ptr(w_hh), ldh, ptr(b), ptr(x), None, 0, None, 0, 0, ptr(h), ptr(c),
                                                    ptr(ho), ptr(c_out), I, H, stream())
    assert call(13, 40, h_out) == -1 and b'multiples of 4' in lib.nnl_last_error()
    assert call(16, 37, h_out) == -1
    assert call(16, 40, h) == -1 and b'alias' in lib.nnl_last_error()
    torch.cuda.synchronize()
    assert float(h_out.min()) == 7.0 and float(c_out.min()) == 7.0
    assert call(16, 40, h_out) == 0
    torch.cuda.synchronize()
    assert float(h_out[:H].abs().max()) == 0.0 and float(h_out[H:].min()) == 7.0      # sigmoid(0) tanh(0) = 0; pad entries untouched


# ---- GPU: nnl_lm_next_token --------------------------------------------------------------------------------------------------------

def _next_token_inputs(V, E, seed, rigged=False):
    g = torch.Generator().manual_seed(7 * V + seed)
    emb = torch.rand(V, E, generator=g, dtype=torch.float64) * 2 - 1
    h = (torch.rand(E, generator=g, dtype=torch.float64) * 2 - 1) * (3.0 / E ** 0.5)        # logits spread over a few units
    if rigged:
        emb[:N_SPECIAL] = h * (6.0 / float(h @ h)) * torch.tensor([1.0, 1.1, 1.2, 1.3], dtype=torch.float64).view(-1, 1)
    u = float(torch.rand(1, generator=g))
    return emb.float().double(), h.float().double(), np.float32(u)


def _drawn_next_token_case(V, E, k, u=None, rigged=False):
    "the first of 50 draws whose margins exceed 100 x the fp32-fp64 distance of its probabilities"
    for seed in range(50):
        emb, h, u_drawn = _next_token_inputs(V, E, seed, rigged)
        uu = u_drawn if u is None else u
        tok, tp, ti, margin = next_token(emb, h, k, uu)
        tok32, tp32, ti32, _ = next_token(emb.float(), h.float(), k, uu)
        d = distance(tp32, tp) if torch.equal(ti, ti32) and tok == tok32 else float('inf')
        if margin > 100 * d:
            return emb, h, uu, tok, tp, ti, d
    raise AssertionError('50 draws gave no case whose margins exceed 100 x the fp32-fp64 distance')


def _run_next_token(emb, h, k, u, with_logits=True):
    from neuralnetworklibrary_amd import ops_text
    V = emb.shape[0]
    tokens = torch.full((5,), -1, dtype=torch.int64, device=DEV)
    top_p, top_i = torch.zeros(3, k, device=DEV), torch.full((3, k), -1, dtype=torch.int64, device=DEV)
    logits = torch.zeros(V, device=DEV) if with_logits else None
    uu = torch.tensor([9.0, 9.0, float(u)], device=DEV)
    ops_text.lm_next_token(emb.float().to(DEV), h.float().to(DEV), k, uu, 2, tokens, 3, top_p, top_i, N_SPECIAL, logits_out=logits)
    assert tokens[:4].tolist() == [-1] * 4 and float(top_p[:2].abs().sum()) == 0.0          # only slot pos + 1 and row `step` are written
    return int(tokens[4]), top_p[2].cpu(), top_i[2].cpu(), None if logits is None else logits.cpu()


def _check_next_token(V, E, k, u=None, rigged=False):
    emb, h, uu, tok, tp, ti, d = _drawn_next_token_case(V, E, k, u, rigged)
    got_tok, got_p, got_i, got_l = _run_next_token(emb, h, k, uu)
    print('next token (%d, %d): |hip - f64| %.2e, torch fp32 %.2e' % (V, k, float((got_p.double() - tp).abs().max()), d))
    assert torch.equal(got_i, ti) and got_tok == tok
    assert float((got_p.double() - tp).abs().max()) <= 10 * d
    l64 = emb @ h
    assert float((got_l.double() - l64).abs().max()) <= 10 * distance(emb.float() @ h.float(), l64)
    assert int(got_i.min()) >= N_SPECIAL
    again = _run_next_token(emb, h, k, uu)
    assert again[0] == got_tok and torch.equal(again[1], got_p) and torch.equal(again[2], got_i)
    return got_tok, got_i


@pytest.mark.gpu
@pytest.mark.parametrize('V,E,k', [(61, 36, 5), (9, 36, 5), (4 + 64, 36, 64), (1000, 36, 1), (47343, 400, 5)])
def test_lm_next_token_vs_fp64(V, E, k):
    """(9, 5): exactly k eligible entries; (68, 64): the largest k; (1000, 1) and (47343, 5): many slices, the last one ragged (V is no
    multiple of 64)"""
    _check_next_token(V, E, k)


@pytest.mark.gpu
def test_lm_next_token_never_picks_a_special_token():
    "a table whose four special rows have the largest logits: they count in the softmax's denominator and are never chosen"
    emb, h, *_ = _drawn_next_token_case(200, 36, 5, rigged=True)
    assert (emb @ h).argsort(descending=True)[:4].sort()[0].tolist() == [0, 1, 2, 3]
    _check_next_token(200, 36, 5, rigged=True)


@pytest.mark.gpu
@pytest.mark.parametrize('u,slot', [(0.0, 0), (1.0 - 2.0 ** -24, -1)])
def test_lm_next_token_extreme_uniforms_pick_first_and_last_slot(u, slot):
    tok, idx = _check_next_token(130, 36, 5, u=np.float32(u))
    assert tok == int(idx[slot])


@pytest.mark.gpu
def test_lm_next_token_argument_errors():
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    V, E = 20, 8
    emb, h, u = torch.zeros(V, E, device=DEV), torch.zeros(E, device=DEV), torch.zeros(1, device=DEV)
    tokens = torch.zeros(2, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1024, device=DEV)
    call = lambda ld, k, wsb: lib.nnl_lm_next_token(ptr(emb), ld, ptr(h), V, E, k, N_SPECIAL, ptr(u), 0, ptr(tokens), 0, None, None, None,
                                                   ptr(ws), wsb, stream())
    assert call(E, 17, 4096) == -1 and call(E, 0, 4096) == -1          # k > V - 4, k < 1
    assert call(E + 1, 5, 4096) == -1                                    # rows not a multiple of 4 floats
    assert call(E, 5, 4) == -4                                           # workspace too small
    assert int(lib.nnl_lm_next_token_workspace_bytes(V, 5)) == 4 * (2 + 2 * 5)
    assert call(E, 5, 4096) == 0
    torch.cuda.synchronize()
    assert int(tokens[1]) == 4                                           # all logits equal: ties go to the lower index, u = 0 picks the first


# ---- GPU: the existing encoder at batch 1 --------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('T,I,H', [(1, 24, 37), (5, 24, 37), (1, 400, 1150), (5, 400, 1150)])
def test_existing_lstm_layer_at_batch_1_vs_fp64(T, I, H):
    "ops_text.lstm_layer forward at B = 1 (tests/lstm_cases.py stops at B = 3); the tolerance of test_text.py's recurrence test"
    from neuralnetworklibrary_amd import ops_text
    g = torch.Generator().manual_seed(T * 10 + H)
    x = torch.randn(T, 1, I, generator=g) * 0.5
    w_ih, w_hh = torch.randn(4 * H, I, generator=g) / I ** 0.5, torch.randn(4 * H, H, generator=g) / H ** 0.5
    b_ih, b_hh = torch.randn(4 * H, generator=g) * 0.1, torch.randn(4 * H, generator=g) * 0.1
    h0, c0 = torch.randn(1, 1, H, generator=g) * 0.1, torch.randn(1, 1, H, generator=g) * 0.1
    dev = lambda t: t.to(DEV)
    with torch.no_grad():
        y, (hT, cT) = ops_text.lstm_layer(dev(x), dev(h0), dev(c0), dev(w_ih), dev(w_hh), dev(b_ih), dev(b_hh))
    yd, (hd, cd) = RT.lstm_layer(x.double(), h0.double(), c0.double(), w_ih.double(), w_hh.double(), b_ih.double(), b_hh.double())
    assert_close(y, yd, 1e-4, 1e-5, 'y')
    assert_close(hT, hd, 1e-4, 1e-5, 'hT')
    assert_close(cT, cd, 1e-4, 1e-5, 'cT')
    from neuralnetworklibrary_amd import ops
    ops.raise_if_index_error()


# ---- GPU: the two loops ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('k', [5, 1])
def test_g20_predict_from_tokens_refeed(g20, g20_net, k):
    "the reference's loop at 400 / 1150 / 3, V = 61: G20's tokens, its probabilities within 10 d (d read from the file)"
    net, _ = g20_net
    net.train()
    toks, probs, idxs = net.predict_from_tokens([int(t) for t in g20['prompt']], int(g20['n']), k=k, seed=int(g20['seed']),
                                                refeed=True, return_probs=True)
    err = float(np.abs(probs.astype(np.float64) - g20['top_probs.k%d.f64' % k]).max())
    print('g20 k = %d: |hip - f64| %.2e, d %.2e' % (k, err, float(g20['d'])))
    assert toks == [int(t) for t in g20['tokens.k%d' % k]]
    assert np.array_equal(idxs, g20['top_indices.k%d' % k])
    assert probs.dtype == np.float32 and idxs.dtype == np.int64 and probs.shape == (int(g20['n']), k)
    assert err <= 10 * float(g20['d'])
    assert net.enc.h[0].shape[1] == net.bs and net.enc.c[2].shape[1] == net.bs
    assert all(float(t.abs().sum()) == 0.0 for t in net.enc.h + net.enc.c)
    assert net.training is False


def _check_incremental(net, P, want=1):
    prompt, n, k = [7, 23, 41, 12, 55], 8, 5
    out = []
    for seed, t64, p64, i64, d in seeds_with_margin(P, prompt, n, k, refeed=False, want=want):
        toks, probs, idxs = net.predict_from_tokens(prompt, n, k=k, seed=seed, refeed=False, return_probs=True)
        print('incremental seed %d: |hip - f64| %.2e, torch fp32 %.2e' % (seed, float(np.abs(probs - p64.numpy()).max()), d))
        assert toks == t64 and np.array_equal(idxs, i64.numpy())
        assert float(np.abs(probs - p64.numpy()).max()) <= 10 * d
        out.append((seed, toks))
    return out


@pytest.mark.gpu
def test_predict_from_tokens_incremental_vs_fp64(g20_net):
    "refeed=False at 400 / 1150 / 3: the prompt through the encoder once, then lstm_cell_b1 per token, against the incremental restatement"
    _check_incremental(*g20_net)


@pytest.mark.gpu
def test_predict_from_tokens_incremental_small_net_and_seeds(small_net):
    """emb 12, hidden 37, 2 layers (nothing a multiple of 64; H needs padding).  One seed twice gives the same tokens; two seeds whose
    restated sequences differ (top-k probabilities not degenerate) differ on the GPU too."""
    net, P = small_net
    prompt, n, k = [7, 23, 41, 12, 55], 8, 5
    cases = seeds_with_margin(P, prompt, n, k, refeed=False, want=6)
    a = cases[0]
    b = next(c for c in cases[1:] if c[1] != a[1])
    got = _check_incremental(net, P, want=6)
    by_seed = dict(got)
    assert by_seed[a[0]] != by_seed[b[0]]
    assert net.predict_from_tokens(prompt, n, k=k, seed=a[0], refeed=False) == by_seed[a[0]]
    one = net.predict_from_tokens(prompt, 1, k=k, seed=a[0], refeed=False)
    assert one == by_seed[a[0]][:len(prompt) + 1]


@pytest.mark.gpu
@pytest.mark.parametrize('refeed', [True, False])
def test_no_host_read_inside_the_loop(g20_net, monkeypatch, refeed):
    "the n steps run under torch.cuda.set_sync_debug_mode('error'): nothing in them waits for the device"
    net, _ = g20_net
    steps = net._generate_steps
    ran = []

    def guarded(*a, **kw):
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode('error')
        try:
            steps(*a, **kw)
            ran.append(1)
        finally:
            torch.cuda.set_sync_debug_mode(before)
    monkeypatch.setattr(net, '_generate_steps', guarded)
    toks = net.predict_from_tokens([7, 23, 41, 12, 55], 6, k=5, seed=3, refeed=refeed)
    assert ran == [1] and len(toks) == 11 and min(toks[5:]) >= N_SPECIAL
