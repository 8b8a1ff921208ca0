"""SENet family on the GPU against golden G24 (tools/gen_golden_senet.py: the real reference on CPU in fp32 and fp64), and the
Dogbreed notebook's call sequence on synthetic images.

The standing rule of tests/test_vision_gpu.py: |hip - f64| <= 3 |ref32 - f64| + 1e-3 |f64| — per tensor in max-norm for the features,
per value for the logits, the loss, the gradient sums and the curve.  The BatchNorm running statistics are taken per tensor in
max-norm like the features: a running mean is a sum of cancelling activations, its absolute error is set by the activations' magnitude
and not by the entry, so an entry near zero has no per-value reference error to scale by.  Every figure is printed before it is
asserted."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from tools.gen_golden_senet import CURVE_LR, STEPS, WD, Data, as_learner_model, batch, build, small_nets

from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.device_data import ImageBatches
from neuralnetworklibrary_amd.Applications.VisionModels import senet
from neuralnetworklibrary_amd.General.Core import separate_bn_layers
from neuralnetworklibrary_amd.General.Learner import Learner

DEV = 'cuda'


@pytest.fixture(scope='module')
def g24():
    return load_golden('g24_senet')


def rule(what, hip, r32, r64, max_norm=False):
    hip, r32, r64 = (np.asarray(a, dtype=np.float64) for a in (hip, r32, r64))
    assert hip.shape == r64.shape, '%s: shape %s vs %s' % (what, hip.shape, r64.shape)
    if max_norm:
        err, allowed = np.abs(hip - r64).max(), 3 * np.abs(r32 - r64).max() + 1e-3 * np.abs(r64).max()
    else:
        err, allowed = np.abs(hip - r64), 3 * np.abs(r32 - r64) + 1e-3 * np.abs(r64)
    print('%-10s worst |hip - f64| / allowed = %.3f' % (what, np.max(err / np.maximum(allowed, 1e-300))))
    assert np.all(err <= allowed), '%s: off the fp64 reference by up to %.3e where %.3e is allowed' % (what, np.max(err), np.max(allowed))


def learner_for(net, tmp_path):
    d = Data()
    d.train_dl = [(None, torch.zeros(Data.bs))]
    d.val_dl = d.train_dl
    learner = Learner(str(tmp_path), d, as_learner_model(net, separate_bn_layers).to(DEV).train(), optimizer='SGD_Mom')
    learner.init_optimizer(wd=WD)
    return learner


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['x', 's'])
def test_g24_eval_train_and_curve_follow_the_reference(g24, key, tmp_path):
    make = small_nets(senet)[key]
    x, y = batch()
    x, y = x.to(DEV), y.to(DEV)
    net = build(make)
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in g24[key + '.param_names']]
    net = net.to(DEV).eval()
    with torch.no_grad():
        feat = net.features(x)
        logits = net.logits(feat)
    rule('features', feat.cpu(), g24[key + '.feat.f32'], g24[key + '.feat.f64'], max_norm=True)
    rule('logits', logits.cpu(), g24[key + '.logits.f32'], g24[key + '.logits.f64'])
    net = build(make).to(DEV).train()
    loss = torch.nn.functional.cross_entropy(net(x), y)
    loss.backward()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    rule('loss', loss.item(), g24[key + '.loss.f32'], g24[key + '.loss.f64'])
    rule('grad sums', [p.grad.double().abs().sum().item() for _, p in net.named_parameters()], g24[key + '.gsum.f32'], g24[key + '.gsum.f64'])
    rule('run. mean', torch.cat([m.running_mean for m in bns]).cpu(), g24[key + '.rmean.f32'], g24[key + '.rmean.f64'], max_norm=True)
    rule('run. var', torch.cat([m.running_var for m in bns]).cpu(), g24[key + '.rvar.f32'], g24[key + '.rvar.f64'], max_norm=True)
    learner = learner_for(build(make), tmp_path)
    curve = [learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(STEPS)]
    print('curve', curve, 'reference fp64', g24[key + '.curve.f64'])
    rule('curve', curve, g24[key + '.curve.f32'], g24[key + '.curve.f64'])


@pytest.mark.gpu
def test_graph_replay_is_bit_equal_to_eager(tmp_path):
    "use_graphs(): after the warm-up the replayed steps' losses and the final parameters equal those of eager steps from the same start"
    make = small_nets(senet)['x']
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


def _decoded(n, seed):
    rs = np.random.RandomState(seed)
    return [{'img': rs.randint(0, 256, (rs.randint(76, 86), rs.randint(76, 86), 3)).astype(np.uint8), 'target': i % 5} for i in range(n)]


@pytest.mark.gpu
def test_dogbreed_call_sequence(tmp_path):
    "ImageClassificationNet -> ImageLearner -> freeze / bn_freeze -> fit -> unfreeze / bn_unfreeze -> data_resize -> fit_cycles -> TTA"
    verbose, Learner.verbose = Learner.verbose, False
    try:
        data = V.ImageDataObj(str(tmp_path), 'single_label', {i: 'breed%d' % i for i in range(5)}, 8, V.get_transforms('SideOn', sz=64),
                              _decoded(24, 0), _decoded(8, 1), seed=3)
        assert isinstance(data.train_dl, ImageBatches)
        torch.manual_seed(0)
        arch = small_nets(senet)['x']()
        model = V.ImageClassificationNet(data, arch)
        assert len(model.layer_groups) == 3
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
        learner.data_resize(96)
        learner.fit_cycles(lr, lr / 100, num_cycles=1)
        assert np.isfinite(learner.loss_sched).all()
        moved = [not torch.equal(a, b) for a, b in zip(body0, model.body.parameters())]
        assert all(moved), '%d body parameters did not move in the unfrozen epoch' % (len(moved) - sum(moved))
        probs, labels = learner.TTA('val')
        assert probs.shape == (8, 5) and np.isfinite(probs).all() and np.abs(probs.sum(1) - 1).max() <= 1e-5
    finally:
        Learner.verbose = verbose


@pytest.mark.gpu
def test_senet154_stage_shapes_run():
    "one SENet-154 block of each stage geometry (groups 64, 3x3 / stride 2 projection shortcut) forward and backward on 2 x 3 x 64 x 64"
    net = small_nets(senet)['s']().to(DEV).train()
    x = torch.randn(2, 3, 64, 64, device=DEV)
    feat = net.features(x)
    assert feat.shape == (2, 2048, 2, 2)
    feat.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in net.named_parameters() if not n.startswith('last_linear'))
