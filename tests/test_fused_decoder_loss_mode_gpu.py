"""The opt-in fused decoder loss above the kernels: Learner.use_fused_decoder_loss() on the tiny AWD-LSTM language-model learner of
tests/test_bf16_linear_mode_gpu.py (same seeds): what it marks, that switching it off restores the step bit for bit, the fused first-step
loss against the use_bf16_linear() one, eval mode, and that no [M, V] buffer is allocated.

First-step bound.  Both routes compute, in fp32, the mean cross-entropy of the SAME bf16-rounded operands (same weights, same masks) plus
the same regulariser, so they differ by at most the sum of their errors against fp64: per row 2 B for each (B = (K + 3) U max_j sum_k
|rb(x)||rb(w)|, test_linear_ce_bf16_gpu.py) + the softmax arithmetic of each: the fused kernels' c_f = 2 R + 2 + 20 T + (ranges + 2)(R + 4)
(ibid.; V = 133: T = 2 tiles, 1 range) and, for softmax_ce_fwd_kernel on 133 columns (one column per lane, then a block reduction of 6
shuffle stages and 4 wave partials, each merge a shift + exp + multiply + add), c_u = R + 2 + 10 (R + 4); for each route + 1 (second
order) + 2 |log s| (logf) + |lse| + |loss| (the two adds); the means: 2 M U mean|loss|; adding the regulariser: 2 U |total|."""
import pytest
import torch

from test_dwconv_gpu import U

from neuralnetworklibrary_amd.Applications.Text import (LanguageModelDecoder, LanguageModelNet, RegSeqCrossEntropyLoss, _Vocab)
from neuralnetworklibrary_amd.General.Core import set_default_device
from neuralnetworklibrary_amd.General.Learner import Learner

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EMB = 24


def _steps(tmp_path, prepare, V=133, bs=3, bptt=5, n=3, watch=None):
    "(the learner, the losses of n steps, the parameters after them) of a freshly seeded language-model learner that `prepare` has set up"
    class Data:
        target_type, stoi = 'lang_model', dict({'tok%d' % i: i for i in range(V) if i != 1}, _pad_=1)
        train_dl = val_dl = [(None, torch.zeros(bs))]
    Data.bs = bs
    set_default_device(DEV)
    torch.manual_seed(0)
    vocab = _Vocab(Data.stoi, bs)
    vocab.target_type = 'lang_model'
    net = LanguageModelNet(vocab, emb_dim=EMB, hidden_size=40, num_layers=2).to(DEV).train()
    learner = Learner(str(tmp_path), Data(), net, optimizer='Adam', loss_func=RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(wd=1e-6, clip=0.4)
    assert prepare(learner) is learner
    if watch is not None:                                               # the decoder's GEMM operands of the first step
        hook = net.dec.drop.register_forward_hook(lambda mod, args, out: watch.setdefault('x', out.detach().clone()))
        watch['w'] = net.dec.lin.weight.detach().clone()
    g = torch.Generator().manual_seed(1)
    stream = torch.randint(2, V, (bs, n * bptt + 1), generator=g).to(DEV)
    watch is not None and watch.update(target=stream[:, 1:bptt + 1])
    torch.manual_seed(2)                                                # the dropout masks and weight-drop seeds of the steps
    losses = []
    for i in range(n):
        if i == n - 1:                                                  # the peak of the last step alone: the optimizer state exists by then
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        losses.append(learner.train1minibatch(stream[:, i * bptt:(i + 1) * bptt].contiguous(), stream[:, i * bptt + 1:(i + 1) * bptt + 1].contiguous(),
                                              [2e-3] * len(net.layer_groups)))
    torch.cuda.synchronize()
    learner.peak = torch.cuda.max_memory_allocated()
    watch is not None and hook.remove()
    return learner, losses, [p.detach().clone() for p in net.parameters()]


def _first_step_bound(watch, total):
    rb = lambda t: t.cpu().bfloat16().double()                                                                                      # noqa: E731
    x, w = rb(watch['x'].reshape(-1, EMB)), rb(watch['w'])
    t = watch['target'].cpu().transpose(0, 1).reshape(-1)
    (M, K), z = x.shape, x @ w.T
    lse, zmax = torch.logsumexp(z, 1), z.max(1).values
    loss = lse - z[torch.arange(M), t]
    B, R = (K + 3) * U * (x.abs() @ w.abs().T).max(1).values, zmax - z.min(1).values
    c_f, c_u = 2 * R + 2 + 20 * 2 + 3 * (R + 4), R + 2 + 10 * (R + 4)
    rows = 4 * B + U * (c_f + c_u + 2 + 2 * (2 * (lse - zmax).abs() + lse.abs() + loss.abs()))
    return float(rows.mean() + 2 * M * U * loss.abs().mean() + 2 * U * abs(total))


def test_use_fused_decoder_loss(tmp_path):
    verbose, Learner.verbose = Learner.verbose, False
    try:
        wf, wb = {}, {}
        plain = _steps(tmp_path, lambda l: l)
        bf16 = _steps(tmp_path, lambda l: l.use_bf16_linear(), watch=wb)
        fused = _steps(tmp_path, lambda l: l.use_bf16_linear().use_fused_decoder_loss(), watch=wf)
        restored = _steps(tmp_path, lambda l: l.use_fused_decoder_loss().use_fused_decoder_loss(False))
        big = {k: _steps(tmp_path, prep, V=20011, bs=16, bptt=32, n=2) for k, prep in      # M = 512 rows: an [M, V] buffer is 41 MB, the model 4 MB
               {'bf16': lambda l: l.use_bf16_linear(), 'fused': lambda l: l.use_bf16_linear().use_fused_decoder_loss()}.items()}
    finally:
        Learner.verbose = verbose
    marked = lambda run: [type(m).__name__ for m in run[0].model.modules() if getattr(m, 'fuse_loss', False)]                      # noqa: E731
    assert marked(fused) == ['LanguageModelDecoder'] and marked(plain) == [] and marked(restored) == []
    assert restored[1] == plain[1] and all(torch.equal(p, q) for p, q in zip(restored[2], plain[2])), 'switching off does not restore the step'
    assert torch.equal(wf['x'], wb['x']) and torch.equal(wf['w'], wb['w']), 'the two first steps saw different operands'
    bound = _first_step_bound(wf, fused[1][0])
    print('losses: fused %r, bf16 linear %r; first step apart by %.3e, bound %.3e' % (fused[1], bf16[1], abs(fused[1][0] - bf16[1][0]), bound))
    assert abs(fused[1][0] - bf16[1][0]) <= bound
    assert all(l == l and abs(l) != float('inf') for l in fused[1]) and all(bool(torch.isfinite(p).all()) for p in fused[2])
    dec = fused[0].model.eval().dec
    assert isinstance(dec, LanguageModelDecoder)
    enc_out = torch.randn(5, 3, EMB, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        pred = dec(enc_out)[0]
        dec.fuse_loss = False
        assert torch.is_tensor(pred) and torch.equal(dec(enc_out)[0], pred), 'eval mode does not materialise the same logits'
    fused[0].model = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match='LanguageModelDecoder'):
        fused[0].use_fused_decoder_loss()
    saved, buffer = big['bf16'][0].peak - big['fused'][0].peak, 16 * 32 * 20011 * 4
    print('peak of one step: bf16 linear %d B, fused %d B: %.2f [M, V] buffers less' % (big['bf16'][0].peak, big['fused'][0].peak, saved / buffer))
    assert saved >= buffer, 'the fused step still holds an [M, V] buffer'
