"""The opt-in bf16 Linear mode above the kernels: Learner.use_bf16_linear() on a tiny AWD-LSTM language-model learner (which modules it marks,
three training steps, and back to the fp32 bits), and the decoder's eval-mode output against ops.linear_bf16 on the same tensors."""
import pytest
import torch

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd.Applications.Text import (LanguageModelDecoder, LanguageModelNet, RegSeqCrossEntropyLoss, WeightDropLSTM1, _Vocab)
from neuralnetworklibrary_amd.General.Core import set_default_device
from neuralnetworklibrary_amd.General.Learner import Learner

pytestmark = pytest.mark.gpu
DEV = 'cuda'
V, BS, BPTT = 133, 3, 5


class Data:
    bs, target_type, stoi = BS, 'lang_model', dict({'tok%d' % i: i for i in range(V) if i != 1}, _pad_=1)
    train_dl = val_dl = [(None, torch.zeros(BS))]


def _steps(tmp_path, prepare):
    "(the learner, the losses of three steps, the parameters after them) of a freshly seeded language-model learner that `prepare` has set up"
    set_default_device(DEV)
    torch.manual_seed(0)
    vocab = _Vocab(Data.stoi, BS)
    vocab.target_type = 'lang_model'
    net = LanguageModelNet(vocab, emb_dim=24, hidden_size=40, num_layers=2).to(DEV).train()
    learner = Learner(str(tmp_path), Data(), net, optimizer='Adam', loss_func=RegSeqCrossEntropyLoss(2.0, 1.0))
    learner.init_optimizer(wd=1e-6, clip=0.4)
    assert prepare(learner) is learner
    g = torch.Generator().manual_seed(1)
    stream = torch.randint(2, V, (BS, 3 * BPTT + 1), generator=g).to(DEV)
    torch.manual_seed(2)                                                # the dropout masks and weight-drop seeds of the three steps
    losses = [learner.train1minibatch(stream[:, i * BPTT:(i + 1) * BPTT].contiguous(), stream[:, i * BPTT + 1:(i + 1) * BPTT + 1].contiguous(),
                                      [2e-3] * len(net.layer_groups)) for i in range(3)]
    return learner, losses, [p.detach().clone() for p in net.parameters()]


def test_use_bf16_linear_marks_trains_and_restores(tmp_path):
    verbose, Learner.verbose = Learner.verbose, False
    try:
        runs = {name: _steps(tmp_path, prep) for name, prep in {
            'fp32': lambda l: l, 'bf16': lambda l: l.use_bf16_linear(), 'restored': lambda l: l.use_bf16_linear().use_bf16_linear(False)}.items()}
    finally:
        Learner.verbose = verbose
    marked = lambda k: [type(m).__name__ for m in runs[k][0].model.modules() if getattr(m, 'compute', None) == 'bf16']               # noqa: E731
    assert marked('bf16') == ['WeightDropLSTM1', 'WeightDropLSTM1', 'LanguageModelDecoder'] and marked('fp32') == [] and marked('restored') == []
    assert all(isinstance(m, (WeightDropLSTM1, LanguageModelDecoder)) == hasattr(m, 'nnl_hip_linear') for m in runs['fp32'][0].model.modules())
    print({k: v[1] for k, v in runs.items()})
    print('bf16 loss curve off the fp32 one by at most %.2e (relative)' % max(abs(a - b) / abs(b) for a, b in zip(runs['bf16'][1], runs['fp32'][1])))
    same = lambda a, b: runs[a][1] == runs[b][1] and all(torch.equal(p, q) for p, q in zip(runs[a][2], runs[b][2]))              # noqa: E731
    assert same('fp32', 'restored'), 'use_bf16_linear(False) does not restore the fp32 path'
    assert runs['bf16'][1] != runs['fp32'][1], 'the bf16 steps are the fp32 ones: the mode reached no kernel'
    assert all(l == l and abs(l) != float('inf') for l in runs['bf16'][1]) and all(bool(torch.isfinite(p).all()) for p in runs['bf16'][2])
    dec = runs['bf16'][0].model.eval().dec
    enc_out = torch.randn(BPTT, BS, 24, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        pred = dec(enc_out)[0]
        direct = ops.linear_bf16(enc_out, dec.lin.weight, None).permute(1, 2, 0)
        dec.compute = 'fp32'
        assert not torch.equal(dec(enc_out)[0], pred), 'the decoder did not leave the fp32 route'
    assert torch.equal(pred, direct), 'the decoder in bf16 mode is not ops.linear_bf16 on its tensors'
