"""NASNet-A-Large on the GPU against golden G27 (tools/gen_golden_nasnet.py: the real reference on CPU in fp32 and fp64), and the
Dogbreed notebook's call sequence on synthetic images.

The rule of tests/test_senet_gpu.py: |hip - f64| <= 3 |ref32 - f64| + 1e-3 |f64| — per tensor in max-norm for activations, input
gradients and BatchNorm running statistics, per value for losses, gradient sums and the curve.  Every figure is printed before it is
asserted.

Gradients and the curve are pinned per cell kind and on the short wiring (one cell of each kind), where the reference's own fp32 and
fp64 runs agree to 1e-6 .. 1e-5.  The full 18-cell class is pinned forward only: its reference fp32 and fp64 weight gradients part by
2 - 30 % per tensor, so a gradient comparison there would either pass vacuously or fail at random."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
from tools.gen_golden_nasnet import (CURVE_LR, FILTERS, N_FULL, PARTS, STEPS, WD, Data, as_learner_model, batch, bn_stats, build,
                                     cell_cases, cell_inputs, cell_weight, full_logits, full_net, short_net)

from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.device_data import ImageBatches
from neuralnetworklibrary_amd.Applications.VisionModels import nasnet
from neuralnetworklibrary_amd.General.Core import separate_bn_layers
from neuralnetworklibrary_amd.General.Learner import Learner

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CELLS = list(cell_cases(nasnet))


@pytest.fixture(scope='module')
def g27():
    out = {}
    for part in PARTS:
        out.update(load_golden(part))
    return out


def rule(what, hip, r64, r32=None, dev32=None):
    "per value with the fp32 run given, per tensor in max-norm with its distance `dev32` from the fp64 run given"
    hip, r64 = (np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64) for a in (hip, r64))
    assert hip.shape == r64.shape, '%s: shape %s vs %s' % (what, hip.shape, r64.shape)
    if dev32 is not None:
        err, allowed = np.abs(hip - r64).max(), 3 * float(dev32) + 1e-3 * np.abs(r64).max()
    else:
        err, allowed = np.abs(hip - r64), 3 * np.abs(np.asarray(r32, dtype=np.float64) - r64) + 1e-3 * np.abs(r64)
    print('%-26s worst |hip - f64| / allowed = %.4f' % (what, np.max(err / np.maximum(allowed, 1e-300))))
    assert np.all(err <= allowed), '%s: off the fp64 reference by up to %.3e where %.3e is allowed' % (what, np.max(err), np.max(allowed))


def stats_rule(g, key, net):
    rmean, rvar = bn_stats(net)
    for what, got in (('rmean', rmean), ('rvar', rvar)):
        r32, r64 = g['%s.%s.f32' % (key, what)], g['%s.%s.f64' % (key, what)]
        rule(key + ' ' + what, got, r64, dev32=np.abs(r32 - r64).max())


@pytest.mark.parametrize('name', CELLS)
def test_each_cell_kind_alone_follows_the_reference(g27, name):
    index = CELLS.index(name)
    make, shapes = cell_cases(nasnet)[name]
    cell = build(make).to(DEV).train()
    xs = [x.to(DEV).requires_grad_(True) for x in cell_inputs(shapes, index)]
    y = cell(*xs)
    (y * cell_weight(y.shape, index).to(DEV)).sum().backward()
    key = 'cell.' + name
    rule(key + ' out', y, g27[key + '.out.f64'], dev32=g27[key + '.out.dev32'])
    for j, x in enumerate(xs):
        rule('%s din%d' % (key, j), x.grad, g27['%s.din%d.f64' % (key, j)], dev32=g27['%s.din%d.dev32' % (key, j)])
    rule(key + ' grad sums', [p.grad.double().abs().sum().item() for _, p in cell.named_parameters()], g27[key + '.gsum.f64'],
         r32=g27[key + '.gsum.f32'])
    stats_rule(g27, key, cell)


def learner_for(net, tmp_path):
    d = Data()
    d.train_dl = [(None, torch.zeros(Data.bs))]
    d.val_dl = d.train_dl
    learner = Learner(str(tmp_path), d, as_learner_model(net, separate_bn_layers).to(DEV).train(), optimizer='SGD_Mom')
    learner.init_optimizer(wd=WD)
    return learner


def test_short_network_eval_train_and_curve_follow_the_reference(g27, tmp_path):
    make = short_net(nasnet)
    x, y = batch()
    x, y = x.to(DEV), y.to(DEV)
    net = build(make).to(DEV).eval()
    with torch.no_grad():
        feat = net.features(x)
    assert feat.shape == (4, 16 * FILTERS, 3, 3)
    rule('short features', feat, g27['short.feat.f64'], dev32=g27['short.feat.dev32'])
    net = build(make).to(DEV).train()
    loss = F.cross_entropy(net(x), y)
    loss.backward()
    rule('short loss', loss.item(), g27['short.loss.f64'], r32=g27['short.loss.f32'])
    rule('short grad sums', [p.grad.double().abs().sum().item() for _, p in net.named_parameters()], g27['short.gsum.f64'],
         r32=g27['short.gsum.f32'])
    stats_rule(g27, 'short', net)
    learner = learner_for(build(make), tmp_path)
    curve = [learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(STEPS)]
    print('curve', curve, 'reference fp64', g27['short.curve.f64'])
    rule('short curve', curve, g27['short.curve.f64'], r32=g27['short.curve.f32'])


def test_short_network_graph_replay_is_bit_equal_to_eager(tmp_path):
    "use_graphs(): after the warm-up the replayed steps' losses and the final parameters equal those of eager steps from the same start"
    make = short_net(nasnet)
    x, y = batch()
    x, y = x.to(DEV), y.to(DEV)
    runs = []
    for graphs in (False, True):
        learner = learner_for(build(make), tmp_path)
        if graphs:
            learner.use_graphs(warmup=2)
        losses = [learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(5)]
        if graphs:
            assert len(learner._graphs) == 1 and next(iter(learner._graphs.values())).graph is not None
        runs.append((losses, [p.detach().clone() for p in learner.model.parameters()]))
    (le, pe), (lg, pg) = runs
    print('eager', le, 'replayed', lg)
    assert le == lg
    assert all(torch.equal(a, b) for a, b in zip(pe, pg))


def test_full_class_forward_follows_the_reference_and_backward_is_finite(g27):
    "forward only (module docstring); one backward with every gradient finite"
    x, y = batch(N_FULL)
    x, y = x.to(DEV), y.to(DEV)
    net = build(full_net(nasnet)).to(DEV).train()
    feat = net.features(x)
    assert feat.shape == (2, 24 * FILTERS, 3, 3) == (2, 576, 3, 3)
    loss = F.cross_entropy(full_logits(net, feat), y)
    rule('full features', feat, g27['full.feat.f64'], dev32=g27['full.feat.dev32'])
    rule('full loss', loss.item(), g27['full.loss.f64'], r32=g27['full.loss.f32'])
    loss.backward()
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)


class ShortBody(nn.Module):
    "the short wiring as a body: what ImageClassificationNet asks of an uncut architecture"

    def __init__(self):
        super().__init__()
        self.net = short_net(nasnet)()
        del self.net.last_linear                                         # (the head is ImageClassificationNet's)
        self.num_features = 16 * FILTERS

    def forward(self, x):
        return self.net.features(x)


def _decoded(n, seed):
    rs = np.random.RandomState(seed)
    return [{'img': rs.randint(0, 256, (rs.randint(76, 86), rs.randint(76, 86), 3)).astype(np.uint8), 'target': i % 5} for i in range(n)]


def test_dogbreed_call_sequence(tmp_path):
    "ImageClassificationNet -> ImageLearner -> freeze / bn_freeze -> fit -> unfreeze / bn_unfreeze -> data_resize -> fit_cycles -> TTA"
    verbose, Learner.verbose = Learner.verbose, False
    try:
        data = V.ImageDataObj(str(tmp_path), 'single_label', {i: 'breed%d' % i for i in range(5)}, 8, V.get_transforms('SideOn', sz=76),
                              _decoded(24, 0), _decoded(8, 1), seed=3)
        assert isinstance(data.train_dl, ImageBatches)
        torch.manual_seed(0)
        model = V.ImageClassificationNet(data, ShortBody())
        assert len(model.layer_groups) == 2                              # an uncut, unsplit body and the head, as for the reference's NASNet
        learner = V.ImageLearner(str(tmp_path), data, model)
        learner.freeze()
        learner.bn_freeze()
        body0 = [p.detach().clone() for p in model.body.parameters()]
        lr = 1e-3
        learner.fit(lr, 1)
        assert len(learner.loss_sched) == 3 and np.isfinite(learner.loss_sched).all()
        assert all(torch.equal(a, b) for a, b in zip(body0, model.body.parameters())), 'a frozen body parameter moved'
        learner.unfreeze()
        learner.bn_unfreeze()
        learner.data_resize(80)                                          # (80 -> 39 -> 20 -> 10: an even map in front of ReductionCell0)
        learner.fit_cycles(lr, lr / 100, num_cycles=1)
        assert np.isfinite(learner.loss_sched).all()
        moved = [not torch.equal(a, b) for a, b in zip(body0, model.body.parameters())]
        assert all(moved), '%d body parameters did not move in the unfrozen epoch' % (len(moved) - sum(moved))
        probs, labels = learner.TTA('val')
        assert probs.shape == (8, 5) and np.isfinite(probs).all() and np.abs(probs.sum(1) - 1).max() <= 1e-5
    finally:
        Learner.verbose = verbose
