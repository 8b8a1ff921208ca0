"""InceptionV4 on the GPU against golden G28 (tools/gen_golden_inception.py: the real reference on CPU in fp32 and fp64), and the
Dogbreed notebook's call sequence on synthetic images.

The rule and helpers of tests/test_nasnet_gpu.py: |hip - f64| <= 3 |ref32 - f64| + 1e-3 |f64| — per tensor in max-norm for activations,
input gradients and running statistics, per value for losses, gradient sums and the curve; figures are printed before they are
asserted.  The full 22-block class only runs: one forward and one backward with every gradient finite."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
from test_nasnet_gpu import rule, stats_rule
from tools.gen_golden_inception import (CURVE_LR, FEATURES, PARTS, STEPS, WD, Data, as_learner_model, batch, block_cases, block_input,
                                        block_weight, build, short_net)

from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import inceptionv4, vmods
from neuralnetworklibrary_amd.General.Core import separate_bn_layers
from neuralnetworklibrary_amd.General.Learner import Learner

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BLOCKS = list(block_cases(inceptionv4))

g28 = pytest.fixture(scope='module')(lambda: {k: v for part in PARTS for k, v in load_golden(part).items()})


def grad_sums(net):
    return [p.grad.double().abs().sum().item() for _, p in net.named_parameters()]


@pytest.mark.parametrize('name', BLOCKS)
def test_each_line_conv_block_alone_follows_the_reference(g28, name):
    index = BLOCKS.index(name)
    make, shape = block_cases(inceptionv4)[name]
    block = build(make).to(DEV).train()
    x = block_input(shape, index).to(DEV).requires_grad_(True)
    y = block(x)
    (y * block_weight(y.shape, index).to(DEV)).sum().backward()
    key = 'block.' + name
    rule(key + ' out', y, g28[key + '.out.f64'], dev32=g28[key + '.out.dev32'])
    rule(key + ' din', x.grad, g28[key + '.din.f64'], dev32=g28[key + '.din.dev32'])
    rule(key + ' grad sums', grad_sums(block), g28[key + '.gsum.f64'], r32=g28[key + '.gsum.f32'])
    stats_rule(g28, key, block)


def learner_for(net, tmp_path):
    d = Data()
    d.train_dl = [(None, torch.zeros(Data.bs))]
    d.val_dl = d.train_dl
    learner = Learner(str(tmp_path), d, as_learner_model(net, separate_bn_layers).to(DEV).train(), optimizer='SGD_Mom')
    learner.init_optimizer(wd=WD)
    return learner


def test_short_network_eval_train_and_curve_follow_the_reference(g28, tmp_path):
    make = short_net(inceptionv4)
    x, y = (t.to(DEV) for t in batch())
    net = build(make).to(DEV).eval()
    with torch.no_grad():
        feat = net.features(x)
    assert feat.shape == (4, FEATURES, 2, 2)
    rule('short features', feat, g28['short.feat.f64'], dev32=g28['short.feat.dev32'])
    net = build(make).to(DEV).train()
    loss = F.cross_entropy(net(x), y)
    loss.backward()
    rule('short loss', loss.item(), g28['short.loss.f64'], r32=g28['short.loss.f32'])
    rule('short grad sums', grad_sums(net), g28['short.gsum.f64'], r32=g28['short.gsum.f32'])
    stats_rule(g28, 'short', net)
    learner = learner_for(build(make), tmp_path)
    curve = [learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(STEPS)]
    rule('short curve', curve, g28['short.curve.f64'], r32=g28['short.curve.f32'])


def test_short_network_graph_replay_is_bit_equal_to_eager(tmp_path):
    x, y = (t.to(DEV) for t in batch())
    runs = []
    for graphs in (False, True):
        learner = learner_for(build(short_net(inceptionv4)), tmp_path)
        if graphs:
            learner.use_graphs(warmup=2)
        losses = [learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(5)]
        if graphs:
            assert len(learner._graphs) == 1 and next(iter(learner._graphs.values())).graph is not None
        runs.append((losses, [p.detach().clone() for p in learner.model.parameters()]))
    (le, pe), (lg, pg) = runs
    assert le == lg
    assert all(torch.equal(a, b) for a, b in zip(pe, pg))


def test_full_class_runs_forward_and_backward():
    x, y = (t.to(DEV) for t in batch(2))
    net = build(lambda: vmods.inceptionv4(num_classes=5)).to(DEV).train()
    logits = net(x)
    assert logits.shape == (2, 5) and bool(torch.isfinite(logits).all())
    F.cross_entropy(logits, y).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


class ShortBody(nn.Module):
    def __init__(self):
        super().__init__()
        self.body = short_net(inceptionv4)().body
        self.num_features = FEATURES

    def forward(self, x):
        return self.body(x)


def _decoded(n, seed):
    rs = np.random.RandomState(seed)
    return [{'img': rs.randint(0, 256, (rs.randint(107, 117), rs.randint(107, 117), 3)).astype(np.uint8), 'target': i % 5} for i in range(n)]


def test_dogbreed_call_sequence(tmp_path):
    verbose, Learner.verbose = Learner.verbose, False
    try:
        data = V.ImageDataObj(str(tmp_path), 'single_label', {i: 'breed%d' % i for i in range(5)}, 8, V.get_transforms('SideOn', sz=107),
                              _decoded(24, 0), _decoded(8, 1), seed=3)
        torch.manual_seed(0)
        model = V.ImageClassificationNet(data, ShortBody())
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
        learner.fit_cycles(lr, lr / 100, num_cycles=1)
        assert np.isfinite(learner.loss_sched).all()
        # The scales of the six BatchNorms that close Inception_C have no gradient while their shifts are 0: relu(g * xhat) = g * relu(xhat)
        # is a per-channel factor, which the head's BatchNorm1d behind the concat pool divides out.  Every other parameter must move.
        scale_free = ['body.10.%s.bn.weight' % b for b in ('branch0', 'branch1_1a', 'branch1_1b', 'branch2_3a', 'branch2_3b', 'branch3.1')]
        still = [n for (n, b), a in zip(model.body.named_parameters(), body0) if torch.equal(a, b) and n not in scale_free]
        assert not still, 'body parameters that did not move in the unfrozen epoch: %s' % still
        probs, labels = learner.TTA('val')
        assert probs.shape == (8, 5) and np.isfinite(probs).all() and np.abs(probs.sum(1) - 1).max() <= 1e-5
    finally:
        Learner.verbose = verbose
