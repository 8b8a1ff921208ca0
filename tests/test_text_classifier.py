"""Text classifier (Applications/Text.py): the length-bucketed data side, the fused attention-pooling kernels of
TextClassificationDecoder (nnl_attn_pool_fwd / _bwd) and the full classifier, pinned to the reference golden G17
(tools/gen_golden_text_classifier.py).  The fp64 restatement of the decoder below is the referee of the GPU tests."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import T, assert_close, load_golden
from oracle import reference_text as RT
from oracle import synth

DEV = 'cuda'


# ---- fp64 restatement of TextClassificationDecoder (reference Text.py:588-609) --------------------------------------------

def _bn_train(x, w, b, eps=1e-5):
    "BatchNorm1d in training mode: batch mean, biased batch variance"
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def ref_fc(p, x, prefix='fc.'):
    "FullyConnectedNet(drops 0, training mode): pre_bn -> (linear -> relu -> bn)* -> final linear (General/Layers.py:89-154)"
    x = _bn_train(x, p[prefix + 'pre_bn.weight'], p[prefix + 'pre_bn.bias'])
    i = 0
    while prefix + 'lins.%d.lin.weight' % i in p:
        q = prefix + 'lins.%d.' % i
        x = _bn_train(F.relu(x @ p[q + 'lin.weight'].t() + p[q + 'lin.bias']), p[q + 'bn.weight'], p[q + 'bn.bias'])
        i += 1
    return x @ p[prefix + 'final_lin.weight'].t() + p[prefix + 'final_lin.bias']


def ref_attention(h, w2, b2, enc, x, pad=1):
    "attn2 -> softmax over ALL t -> pad mask -> renormalise -> weighted sum, as the reference writes it: (attn [T,B], pooled [B,E])"
    s = (h @ w2.reshape(-1, 1) + b2).squeeze(2)
    a = F.softmax(s, dim=0) * (x.transpose(1, 0) != pad).to(h.dtype)
    a = a / a.sum(dim=0).unsqueeze(0)
    return a, (a.unsqueeze(2) * enc).sum(0)


def ref_decoder(p, x, enc, prefix=''):
    "TextClassificationDecoder.forward with parameters p (name -> tensor): (pred, attn)"
    h = F.relu(enc @ p[prefix + 'attn1.weight'].t() + p[prefix + 'attn1.bias'])
    attn, pooled = ref_attention(h, p[prefix + 'attn2.weight'], p[prefix + 'attn2.bias'], enc, x)
    return ref_fc(p, pooled, prefix + 'fc.'), attn


def _g17a_params(g, dtype=torch.float64):
    from neuralnetworklibrary_amd.Applications.Text import TextClassificationDecoder
    dec = TextClassificationDecoder(16, 3, 12, [10], [0., 0.])
    synth.fill_module_(dec, seed=17)
    assert [n for n, _ in dec.named_parameters()] == [str(s) for s in g['a.param_names']]
    return dec, {n: p.detach().to(dtype).clone().requires_grad_(True) for n, p in dec.named_parameters()}


def _g17a_loss(g, pred, attn, dev='cpu', dtype=torch.float64):
    B, C = pred.shape
    return (pred * synth.synth_input((B, C), 1703).to(dev, dtype)).sum() + (attn * synth.synth_input(tuple(attn.shape), 1704).to(dev, dtype)).sum()


# ---- CPU: data side -----------------------------------------------------------------------------------------------------

def _g17b_texts(g):
    lengths, tokens = g['b.lengths'], g['b.tokens']
    offs = np.concatenate([[0], np.cumsum(lengths)])
    return [list(tokens[offs[i]:offs[i + 1]]) for i in range(len(lengths))], [str(s) for s in g['b.labels']]


def test_g17_sampler_permutes_dataset_and_batches_like_the_reference():
    from neuralnetworklibrary_amd.Applications.Text import TextDataset, TextLengthSampler
    g = load_golden('g17_text_classifier')
    texts, labels = _g17b_texts(g)
    bs, bpg = int(g['b.bs']), int(g['b.bpg'])
    for tag, random in (('fixed', False), ('random', True)):
        ds = TextDataset(texts, labels, stoi={'_pad_': 1})
        assert ds.label_dict == {'mid': 0, 'neg': 1, 'pos': 2} and ds.num_tokens == sum(len(t) for t in texts)
        np.random.seed(1712)
        s = TextLengthSampler(ds, bs, bpg, random=random)
        batches = [list(b) for b in s]
        assert len(s) == int(g['b.%s.len' % tag])
        assert ds.perm == list(g['b.%s.perm' % tag])
        assert [len(b) for b in batches] == list(g['b.%s.batch_sizes' % tag])
        assert np.concatenate(batches).tolist() == g['b.%s.batches' % tag].tolist()
        assert list(ds.labels) == list(g['b.%s.sorted_labels' % tag])
        assert [len(t) for t in ds.texts] == sorted([len(t) for t in texts], reverse=True)
        assert list(ds.texts.index) == list(range(len(texts)))


def test_g17_collater_pads_at_the_end_on_the_host():
    from neuralnetworklibrary_amd.Applications.Text import TextDataset, TextLengthCollater, TextLengthSampler
    g = load_golden('g17_text_classifier')
    texts, labels = _g17b_texts(g)
    ds = TextDataset(texts, labels, stoi={'_pad_': 1})
    TextLengthSampler(ds, int(g['b.bs']), int(g['b.bpg']))
    x, y = TextLengthCollater(1)([ds[i] for i in (5, 6, 7)])
    assert x.dtype == torch.int64 and y.dtype == torch.int64 and not x.is_cuda and not y.is_cuda
    assert x.tolist() == g['b.collate.x'].tolist() and y.tolist() == g['b.collate.y'].tolist()


def test_g17_data_object_loaders_match_the_reference():
    from neuralnetworklibrary_amd.Applications.Text import TextClassificationDataObj, TextDataset
    g = load_golden('g17_text_classifier')
    texts, labels = _g17b_texts(g)
    tr, va = TextDataset(texts, labels, stoi={'_pad_': 1}), TextDataset(texts[:11], labels[:11], stoi={'_pad_': 1})
    np.random.seed(1713)
    d = TextClassificationDataObj(tr, va, None, int(g['b.bs']), int(g['b.bpg']), num_workers=0)
    assert d.target_type == 'text_classify' and d.stoi == {'_pad_': 1} and not hasattr(d, 'test_dl')
    xs = [(x.numpy(), y.numpy()) for x, y in d.train_dl]
    assert np.array([x.shape for x, _ in xs]).tolist() == g['b.obj.train_shapes'].tolist()
    assert np.concatenate([x.reshape(-1) for x, _ in xs]).tolist() == g['b.obj.train_x'].tolist()
    assert np.concatenate([y for _, y in xs]).tolist() == g['b.obj.train_y'].tolist()
    assert np.concatenate([y.numpy() for _, y in d.val_dl]).tolist() == g['b.obj.val_y'].tolist()


def test_dataset_reverse_and_split_train_val():
    from neuralnetworklibrary_amd.Applications.Text import TextDataset
    ds = TextDataset([[4, 5, 6], [7, 8], [9], [10, 11, 12, 13], [14, 15]], [1, 0, 1, 1, 0], reverse=True)
    assert ds.texts.tolist() == [[6, 5, 4], [8, 7], [9], [13, 12, 11, 10], [15, 14]] and ds.reverse
    assert ds[3] == ([13, 12, 11, 10], 1)
    np.random.seed(3)
    tr, va = ds.split_train_val()
    assert len(tr) + len(va) == 5 and len(va) == 1
    assert tr.num_tokens + va.num_tokens == 12
    assert sorted(tr.texts.tolist() + va.texts.tolist()) == sorted([[6, 5, 4], [8, 7], [9], [13, 12, 11, 10], [15, 14]])


def test_tokenising_paths_raise_not_implemented():
    from neuralnetworklibrary_amd.Applications.Text import TextClassificationDataObj, TextDataset
    with pytest.raises(NotImplementedError):
        TextDataset(['a raw string needs spaCy'], [0])
    with pytest.raises(NotImplementedError):
        TextDataset.from_csv('train.csv', 'text', 'label')
    with pytest.raises(NotImplementedError):
        TextDataset.from_text_files('train', ['neg', 'pos'])
    with pytest.raises(NotImplementedError):
        TextClassificationDataObj.from_csv(16, 'train.csv')
    with pytest.raises(NotImplementedError):
        TextClassificationDataObj.from_folders(16, ['neg', 'pos'], 'train')


# ---- CPU: the restatement against the reference, and the C entry points' argument checks --------------------------------

def test_g17_decoder_restatement_fp64_matches_the_reference():
    g = load_golden('g17_text_classifier')
    _, p = _g17a_params(g)
    enc = T(g['a.enc']).double().requires_grad_(True)
    pred, attn = ref_decoder(p, T(g['a.x']), enc)
    assert_close(pred, g['a.pred'], 1e-5, 1e-6, 'pred')
    assert_close(attn, g['a.attn'], 1e-5, 1e-7, 'attn')
    _g17a_loss(g, pred, attn).backward()
    assert_close(enc.grad, g['a.d_enc'], 1e-4, 1e-6, 'd enc_out')
    for n, t in p.items():
        assert_close(t.grad, g['a.grad.' + n], 1e-4, 1e-6, 'grad ' + n)


def test_attn_pool_entry_points_reject_bad_arguments_before_any_hip_call():
    from neuralnetworklibrary_amd import _lib
    lib = _lib.lib
    fake = C.c_void_p(4096)                         # never dereferenced: every call below fails its argument checks first
    cnt = (C.c_int32 * 8)()
    assert lib.nnl_attn_pool_workspace_bytes(0, 4, 8, 8) == 0
    assert lib.nnl_attn_pool_workspace_bytes(5, 4, 7, 3) > 0
    ws_need = int(lib.nnl_attn_pool_workspace_bytes(5, 4, 8, 8))
    fwd = lambda *a: lib.nnl_attn_pool_fwd(*a)
    args = [fake, fake, fake, fake, fake, 1, fake, fake, 5, 4, 8, 8, fake, ws_need, C.cast(cnt, C.c_void_p), 8, None]
    for i in range(8):
        if i == 5:
            continue
        bad = list(args)
        bad[i] = None
        assert fwd(*bad) == -1, 'fwd null pointer %d' % i
    for i, v in ((8, 0), (9, 0), (10, 0), (11, -3), (9, 1 << 31)):
        bad = list(args)
        bad[i] = v
        assert fwd(*bad) == -1, 'fwd size %d = %d' % (i, v)
    bad = list(args); bad[15] = 4                    # B + 1 = 5 counters needed
    assert fwd(*bad) == -1 and b'counters' in lib.nnl_last_error()
    bad = list(args); bad[13] = ws_need - 4
    assert fwd(*bad) == -4
    bad = list(args); bad[12] = None
    assert fwd(*bad) == -4
    bad = list(args); bad[12] = C.c_void_p(4100)
    assert fwd(*bad) == -1 and b'aligned' in lib.nnl_last_error()
    bwd_args = [fake, fake, fake, fake, fake, None, fake, fake, fake, fake, 5, 4, 8, 8, fake, ws_need, C.cast(cnt, C.c_void_p), 8, None]
    for i in (0, 1, 2, 3, 4, 6, 7, 8, 9):
        bad = list(bwd_args)
        bad[i] = None
        assert lib.nnl_attn_pool_bwd(*bad) == -1, 'bwd null pointer %d' % i
    bad = list(bwd_args); bad[13] = 0
    assert lib.nnl_attn_pool_bwd(*bad) == -1
    bad = list(bwd_args); bad[15] = 16
    assert lib.nnl_attn_pool_bwd(*bad) == -4


# ---- GPU: the kernels against the restatement ----------------------------------------------------------------------------

def _pool_case(Tn, B, E, A, seed, all_pad_col=None):
    g = torch.Generator().manual_seed(seed)
    h = torch.relu(torch.randn(Tn, B, A, generator=g))
    w2, b2 = torch.randn(1, A, generator=g) / A ** 0.5, torch.randn(1, generator=g)
    enc = torch.randn(Tn, B, E, generator=g)
    lengths = torch.randint(1, Tn + 1, (B,), generator=g)
    lengths[0] = Tn
    x = torch.randint(2, 100, (B, Tn), generator=g)
    x[torch.arange(Tn)[None, :] >= lengths[:, None]] = 1               # ragged rows, end-padded with 1
    x[:, 0][torch.rand(B, generator=g) < 0.2] = 1                        # and a few pads in the middle of a row
    x[torch.arange(B), lengths - 1] = 3                                  # every row keeps a non-pad token
    if all_pad_col is not None:
        x[all_pad_col] = 1
    return h, w2, b2, enc, x


@pytest.mark.gpu
@pytest.mark.parametrize('Tn,B,E,A', [(2, 2, 4, 1), (7, 5, 18, 13), (33, 3, 400, 50), (75, 64, 400, 100), (300, 64, 400, 100),
                                      (1000, 64, 400, 100), (2048, 8, 400, 100)])
@pytest.mark.parametrize('with_dattn', [False, True])
def test_attention_pool_vs_fp64_restatement(Tn, B, E, A, with_dattn):
    from neuralnetworklibrary_amd import ops_text
    h, w2, b2, enc, x = _pool_case(Tn, B, E, A, 1000 * Tn + B)
    g = torch.Generator().manual_seed(7)
    dpooled, dattn = torch.randn(B, E, generator=g), torch.randn(Tn, B, generator=g)
    ref = [t.double().requires_grad_(True) for t in (h, w2, b2, enc)]
    ra, rp = ref_attention(*ref, x)
    ((rp * dpooled.double()).sum() + ((ra * dattn.double()).sum() if with_dattn else 0)).backward()
    dev = [t.to(DEV).requires_grad_(True) for t in (h, w2, b2, enc)]
    attn, pooled = ops_text.attention_pool(*dev, x.to(DEV))
    loss = (pooled * dpooled.to(DEV)).sum() + ((attn * dattn.to(DEV)).sum() if with_dattn else 0)
    loss.backward()
    assert_close(attn, ra, 1e-5, 1e-7, 'attn')
    assert_close(pooled, rp, 1e-5, 1e-6, 'pooled')
    for name, d, r in zip(('dh', 'dw2', 'denc'), (dev[0], dev[1], dev[3]), (ref[0], ref[1], ref[3])):
        scale = r.grad.abs().max().item()
        assert d.grad.shape == r.grad.shape, name
        assert_close(d.grad, r.grad, 1e-4, 1e-5 * max(scale, 1e-3), name)
    # db2 = sum of dlogit = 0 up to rounding (a shift of every score cancels in the softmax): judged against sum |dlogit|
    with torch.no_grad():
        gg = (ref[3] * dpooled.double()).sum(2) + (dattn.double() if with_dattn else 0)
        dlogit = ra * (gg - (ra * gg).sum(0))
    assert dev[2].grad.shape == ref[2].grad.shape
    assert abs(dev[2].grad.item() - ref[2].grad.item()) <= 2e-5 * dlogit.abs().sum().item() + 1e-9, (dev[2].grad, ref[2].grad)


@pytest.mark.gpu
def test_attention_pool_bitwise_repeatable_and_all_pad_column_is_nan():
    from neuralnetworklibrary_amd import ops_text
    h, w2, b2, enc, x = _pool_case(1000, 64, 400, 100, 5, all_pad_col=17)
    dev = [t.to(DEV).requires_grad_(True) for t in (h, w2, b2, enc)]
    dpooled = torch.randn(64, 400, generator=torch.Generator().manual_seed(3)).to(DEV)
    dpooled[17] = 0
    runs = []
    for _ in range(3):
        for t in dev:
            t.grad = None
        attn, pooled = ops_text.attention_pool(*dev, x.to(DEV))
        (pooled[torch.arange(64, device=DEV) != 17] * dpooled[torch.arange(64, device=DEV) != 17]).sum().backward()
        runs.append([attn.detach().clone(), pooled.detach().clone()] + [t.grad.clone() for t in dev])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)) and torch.equal(a.isnan(), b.isnan())
    attn, pooled = runs[0][0], runs[0][1]
    assert attn[:, 17].isnan().all() and pooled[17].isnan().all()
    keep = torch.arange(64, device=DEV) != 17
    assert not attn[:, keep].isnan().any() and not pooled[keep].isnan().any()
    assert_close(attn[:, keep].sum(0), torch.ones(63), 1e-5, 1e-5, 'columns sum to 1')
    assert (attn[x.to(DEV).t() == 1] == 0)[(~attn[x.to(DEV).t() == 1].isnan())].all()


# ---- GPU: goldens -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_g17_decoder_hip():
    g = load_golden('g17_text_classifier')
    dec, _ = _g17a_params(g)
    dec = dec.to(DEV).train()
    enc = T(g['a.enc'], DEV).requires_grad_(True)
    pred, attn = dec(T(g['a.x'], DEV), enc)
    assert_close(pred, g['a.pred'], 1e-4, 1e-5, 'pred')
    assert_close(attn, g['a.attn'], 1e-5, 1e-7, 'attn')
    _g17a_loss(g, pred, attn, DEV, torch.float32).backward()
    assert_close(enc.grad, g['a.d_enc'], 1e-3, 1e-5, 'd enc_out')
    for n, p in dec.named_parameters():
        assert_close(p.grad, g['a.grad.' + n], 1e-3, 1e-5, 'grad ' + n)


def _product_classifier(V, bs, path='/tmp/nnl_test_g17'):
    from neuralnetworklibrary_amd.Applications.Text import LanguageModelNet, TextClassificationNet, _Vocab
    stoi = {('tok%d' % i): i for i in range(V)}
    stoi['_pad_'] = 1
    del stoi['tok1']
    lm = LanguageModelNet(_Vocab(stoi, bs), enc_drops=[0., 0., 0., 0.], dec_drop=0.)
    synth.fill_lm_reference_init_(lm, seed=17)
    net = TextClassificationNet(path, lm, 3, enc_drops=[0., 0., 0., 0.], fc_drops=[0., 0.])
    synth.fill_module_(net.dec, seed=18)
    return net.to(DEV).train()


@pytest.mark.gpu
def test_g17_full_size_classifier_forward_backward_and_learner_steps():
    from functools import partial
    from neuralnetworklibrary_amd.Applications.Text import RegSeqCrossEntropyLoss
    from neuralnetworklibrary_amd.General.Learner import Learner
    from neuralnetworklibrary_amd.General.Optimizer import Optimizer
    g = load_golden('g17_text_classifier')
    net = _product_classifier(60, 4)
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in g['c.param_names']]
    lf = RegSeqCrossEntropyLoss(2.0, 1.0)
    out = net(T(g['c.x0'], DEV))
    loss = lf(out, T(g['c.y0'], DEV))
    loss.backward()
    assert_close(loss, g['c.loss'], 1e-4, 1e-6, 'loss')
    assert_close(lf.cross_entropy, g['c.ce'], 1e-4, 1e-6, 'ce')
    assert_close(out[0], g['c.pred'], 1e-4, 1e-5, 'pred')
    norms = np.array([p.grad.norm().item() for p in net.parameters()])
    assert_close(norms, g['c.grad_norms'], 2e-3, 1e-7, 'gradient norms')
    sd = dict(net.named_parameters())
    for name, got, key in (('attn1', sd['dec.attn1.weight'].grad[:16, :64], 'c.grad.attn1_slice'),
                           ('attn2', sd['dec.attn2.weight'].grad, 'c.grad.attn2'),
                           ('embedding', sd['enc.word_embed.embed.weight'].grad, 'c.grad.emb'),
                           ('whh2', sd['enc.lstms.2.lstm.weight_hh_l0_raw'].grad[:64, :64], 'c.grad.whh2_slice')):
        ref = torch.from_numpy(g[key]).double()       # normwise: single elements of these gradients are sums with cancellation
        err = (got.detach().cpu().double() - ref).norm().item()
        assert err <= 2e-3 * ref.norm().item(), '%s grad: |hip - ref| %.3e vs |ref| %.3e' % (name, err, ref.norm().item())

    class D:
        bs, target_type = 4, 'text_classify'
    net = _product_classifier(60, 4)
    batches = [(T(g['c.x%d' % i], DEV), T(g['c.y%d' % i], DEV)) for i in range(2)]
    D.train_dl = D.val_dl = batches
    learner = Learner('/tmp/nnl_test_g17', D(), net, Optimizer(partial(torch.optim.Adam, betas=(0.7, 0.99)), net),
                      RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(clip=1.0)
    net.train()
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    losses = [learner.train1minibatch(x, y, [2e-4, 1e-3, 5e-3], betas_batch=(0.7, 0.99)) for x, y in batches]
    assert_close(np.array(losses), g['c.step_losses'], 1e-4, 1e-6, 'step losses')
    # attn2.bias, and attn1.bias where a unit's ReLU is open at every position, have an exact gradient of 0 (sum_t dlogit = 0 per
    # column: a shift of the scores cancels in the softmax), so Adam's first updates there are +-lr times the sign of rounding noise,
    # in the reference's own run as much as here.  Those two are held to Adam's step bound; every other parameter to the golden.
    noisy = ('dec.attn1.bias', 'dec.attn2.bias')
    names = [str(s) for s in g['c.param_names']]
    sums = np.array([p.double().abs().sum().item() for p in net.parameters()])
    keep = [i for i, n in enumerate(names) if n not in noisy]
    assert_close(sums[keep], g['c.after.abs_sums'][keep], 1e-4, 1e-7, 'abs sums')
    for n in noisy:
        step = (dict(net.named_parameters())[n].detach() - before[n]).abs().max().item()
        assert step <= 2 * 5e-3 * 1.01, (n, step)


@pytest.mark.gpu
def test_g17_ten_step_loss_curve_every_step_within_1e3():
    from functools import partial
    from neuralnetworklibrary_amd.Applications.Text import RegSeqCrossEntropyLoss
    from neuralnetworklibrary_amd.General.Learner import Learner
    from neuralnetworklibrary_amd.General.Optimizer import Optimizer
    g = load_golden('g17_text_classifier')
    V, bs, steps = int(g['d.V']), int(g['d.bs']), int(g['d.steps'])
    net = _product_classifier(V, bs)

    class D:
        target_type = 'text_classify'
    D.bs = bs
    D.train_dl = D.val_dl = [(None, torch.zeros(bs))]
    learner = Learner('/tmp/nnl_test_g17', D(), net, Optimizer(partial(torch.optim.Adam, betas=(0.7, 0.99)), net),
                      RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(clip=1.0)
    net.train()
    losses = []
    for i in range(steps):
        x, y = T(g['d.x%d' % i].astype(np.int64), DEV), T(g['d.y%d' % i], DEV)
        losses.append(learner.train1minibatch(x, y, [float(v) for v in g['d.lr']], betas_batch=(0.7, 0.99)))
    ref = g['d.losses.f32']
    rel = np.abs(np.array(losses) - ref) / np.abs(ref)
    print('hip vs ref32 per step:', np.array2string(rel, precision=1))
    assert (rel <= 1e-3).all(), 'loss curve: %s vs %s' % (losses, ref.tolist())


# ---- GPU: long sequences through the whole classifier, against the CPU oracle ---------------------------------------------

@pytest.mark.gpu
def test_full_size_classifier_long_sequences_vs_oracle_fp64():
    """The 400 / 1150 / 3 classifier at bs 16, T = 600 (ragged, end-padded): one forward + RegSeqCrossEntropyLoss(2, 1) + backward
    against the CPU oracle (oracle/reference_text.py's encoder + the fp64 restatement of the decoder above) in fp32 and fp64.
    Per parameter gradient: ||hip - f64|| <= 3 ||cpu32 - f64|| + 1e-3 ||f64||; loss likewise."""
    V, bs, Tn = 200, 16, 600
    net = _product_classifier(V, bs)
    names = [n for n, _ in net.named_parameters()]
    sd = {n: p.detach().cpu() for n, p in net.named_parameters()}
    gen = torch.Generator().manual_seed(21)
    lengths = torch.randint(Tn // 2, Tn + 1, (bs,), generator=gen)
    lengths[0] = Tn
    x = torch.randint(4, V, (bs, Tn), generator=gen)
    x[torch.arange(Tn)[None, :] >= lengths[:, None]] = 1
    y = torch.randint(0, 3, (bs,), generator=gen)
    from neuralnetworklibrary_amd.Applications.Text import RegSeqCrossEntropyLoss
    lf = RegSeqCrossEntropyLoss(2.0, 1.0)
    loss_p = lf(net(x.to(DEV)), y.to(DEV))
    loss_p.backward()
    results = {}
    for dtype in (torch.float32, torch.float64):
        enc = RT.LSTM_Encoder(V, 400, 1150, 3, 1, bs).to(dtype)
        enc.load_state_dict({k[4:]: v.to(dtype) for k, v in sd.items() if k.startswith('enc.')})
        enc.h, enc.c = [t.to(dtype) for t in enc.h], [t.to(dtype) for t in enc.c]
        dec = {k[4:]: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith('dec.')}
        enc_out = enc(x)
        pred, _ = ref_decoder(dec, x, enc_out)
        loss, _ = RT.reg_seq_cross_entropy((pred, enc_out), y, 2.0, 1.0)
        loss.backward()
        grads = {('enc.' + n): p.grad for n, p in enc.named_parameters()}
        grads.update({('dec.' + n): p.grad for n, p in dec.items()})
        results[dtype] = (loss.item(), grads)
    (l32, g32), (l64, g64) = results[torch.float32], results[torch.float64]
    assert abs(loss_p.item() - l64) <= 3 * abs(l32 - l64) + 1e-3 * abs(l64), (loss_p.item(), l32, l64)
    worst = 0.0
    for n, p in zip(names, net.parameters()):
        if n == 'dec.attn2.bias':
            # exactly 0 (a shift of every score cancels in the softmax): only rounding remains, judged in absolute terms
            assert abs(p.grad.item()) <= 1e-4 and abs(g32[n].item()) <= 1e-4, (p.grad, g32[n])
            continue
        gp, c32, c64 = p.grad.detach().cpu().double(), g32[n].double(), g64[n]
        e_hip, e_cpu, ref = (gp - c64).norm().item(), (c32 - c64).norm().item(), c64.norm().item()
        worst = max(worst, e_hip / max(ref, 1e-300))
        assert e_hip <= 3 * e_cpu + 1e-3 * ref, '%s: |hip-f64| %.3e vs |cpu32-f64| %.3e (|f64| %.3e)' % (n, e_hip, e_cpu, ref)
    print('worst relative gradient error vs fp64: %.2e' % worst)


# ---- GPU: end to end ------------------------------------------------------------------------------------------------------

def _marker_texts(n, rs, V=40, marker=5):
    lengths = rs.randint(6, 60, n)
    labels = rs.randint(0, 2, n)
    texts = []
    for L, lab in zip(lengths, labels):
        t = rs.randint(6, V, L)
        if lab:
            t[rs.randint(0, L)] = marker
        texts.append(list(t))
    return texts, ['yes' if lab else 'no' for lab in labels]


@pytest.mark.gpu
@pytest.mark.parametrize('seed', [0, 1])
def test_end_to_end_classifier_learns_marker_task_and_predicts_in_permuted_order(seed, tmp_path):
    from neuralnetworklibrary_amd.Applications.Text import (LanguageModelNet, RegSeqCrossEntropyLoss, TextClassificationDataObj,
                                                            TextClassificationNet, TextDataset, _Vocab)
    from neuralnetworklibrary_amd.General.Learner import Learner
    torch.manual_seed(seed)
    np.random.seed(seed)
    rs = np.random.RandomState(100 + seed)
    V, bs = 40, 32
    stoi = {('tok%d' % i): i for i in range(V)}
    stoi['_pad_'] = 1
    del stoi['tok1']
    (trt, trl), (vat, val), (tet, tel) = _marker_texts(640, rs), _marker_texts(96, rs), _marker_texts(160, rs)
    train_ds, val_ds, test_ds = (TextDataset(t, l, stoi=stoi) for t, l in ((trt, trl), (vat, val), (tet, tel)))
    data = TextClassificationDataObj(train_ds, val_ds, test_ds, bs, num_workers=0)
    lm = LanguageModelNet(_Vocab(stoi, bs), emb_dim=32, hidden_size=64, num_layers=2)
    net = TextClassificationNet(str(tmp_path), lm, 2, attn_size=16, fc_layer_sizes=[16], fc_drops=[0.1, 0.1])
    learner = Learner(str(tmp_path), data, net, optimizer='Adam', loss_func=RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.freeze()
    learner.fit([3e-3, 3e-3, 3e-3], 1)
    learner.unfreeze()
    learner.fit_one_cycle([3e-3, 3e-3, 1e-2], 6, clip=1.0)
    learner.save('clf')
    learner.load('clf')
    probs, preds = learner.predict('test')
    assert probs.shape == (160, 2)
    truth = np.array(test_ds.labels)                     # permuted by the test sampler (longest first), as predict() is
    assert [len(t) for t in test_ds.texts] == sorted([len(t) for t in tet], reverse=True)
    assert truth.tolist() == [test_ds.label_dict[tel[i]] for i in test_ds.perm]
    acc = (preds == truth).mean()
    print('seed %d: test accuracy %.3f' % (seed, acc))
    assert acc >= 0.9, acc
