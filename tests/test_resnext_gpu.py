"""ResNeXt-101 on the GPU against golden G29 (tools/gen_golden_resnext.py: the real reference in fp32 and fp64, cut to the stem and the first
block of every stage) under the rule of tests/test_senet_gpu.py (imported): |hip - f64| <= 3 |ref32 - f64| + 1e-3 |f64|, max-norm for features
and running statistics.  Then the full networks: the Dogbreed call sequence on synthetic images for 32x4d, one forward at 224 x 224 for 64x4d."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_senet_gpu import DEV, _decoded, learner_for, rule
from tools.gen_golden_resnext import CURVE_LR, NCLS, STEPS, batch, build

from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import resnext, vmods
from neuralnetworklibrary_amd.General.Learner import Learner

SHORT = {k: (lambda cls=cls: cls(num_classes=NCLS, stages=(1, 1, 1, 1))) for k, cls in (('32', resnext.ResNeXt101_32x4d), ('64', resnext.ResNeXt101_64x4d))}


@pytest.fixture(scope='module')
def g29():
    return load_golden('g29_resnext')


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['32', '64'])
def test_g29_eval_train_and_curve_follow_the_reference(g29, key, tmp_path):
    make = SHORT[key]
    x, y = (t.to(DEV) for t in batch())
    net = build(make)
    assert len(list(net.parameters())) == len(g29[key + '.param_names'])          # matched by position
    net = net.to(DEV).eval()
    with torch.no_grad():
        feat = net.features(x)
        logits = net.logits(feat)
    rule('features', feat.cpu(), g29[key + '.feat.f32'], g29[key + '.feat.f64'], max_norm=True)
    rule('logits', logits.cpu(), g29[key + '.logits.f32'], g29[key + '.logits.f64'])
    net = build(make).to(DEV).train()
    loss = torch.nn.functional.cross_entropy(net(x), y)
    loss.backward()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    rule('loss', loss.item(), g29[key + '.loss.f32'], g29[key + '.loss.f64'])
    rule('grad sums', [p.grad.double().abs().sum().item() for _, p in net.named_parameters()], g29[key + '.gsum.f32'], g29[key + '.gsum.f64'])
    rule('run. mean', torch.cat([m.running_mean for m in bns]).cpu(), g29[key + '.rmean.f32'], g29[key + '.rmean.f64'], max_norm=True)
    rule('run. var', torch.cat([m.running_var for m in bns]).cpu(), g29[key + '.rvar.f32'], g29[key + '.rvar.f64'], max_norm=True)
    runs = []
    for graphs in (False, True):
        learner = learner_for(build(make), tmp_path)
        if graphs:
            learner.use_graphs(warmup=2)
        runs.append([learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(STEPS)])
    print('curve', runs[0], 'replayed', runs[1], 'reference fp64', g29[key + '.curve.f64'])
    rule('curve', runs[0], g29[key + '.curve.f32'], g29[key + '.curve.f64'])
    assert runs[0] == runs[1], 'use_graphs() replay differs from the eager steps'


@pytest.mark.gpu
def test_full_networks_train_and_run(tmp_path, monkeypatch):
    "resnext101_32x4d: ImageClassificationNet -> ImageLearner -> freeze -> fit -> unfreeze -> fit; resnext101_64x4d: one forward at 224"
    monkeypatch.setattr(Learner, 'verbose', False)
    data = V.ImageDataObj(str(tmp_path), 'single_label', {i: 'breed%d' % i for i in range(5)}, 8, V.get_transforms('SideOn', sz=64),
                          _decoded(16, 0), _decoded(8, 1), seed=3)
    torch.manual_seed(0)
    model = V.ImageClassificationNet(data, vmods.resnext101_32x4d())
    learner = V.ImageLearner(str(tmp_path), data, model)
    learner.freeze()
    learner.bn_freeze()
    body0 = [p.detach().clone() for p in model.body.parameters()]
    learner.fit(1e-3, 1)
    assert np.isfinite(learner.loss_sched).all()
    assert all(torch.equal(a, b) for a, b in zip(body0, model.body.parameters())), 'a frozen body parameter moved'
    learner.unfreeze()
    learner.bn_unfreeze()
    learner.fit(1e-3, 1)
    assert np.isfinite(learner.loss_sched).all()
    moved = [not torch.equal(a, b) for a, b in zip(body0, model.body.parameters())]
    assert all(moved), '%d body parameters did not move in the unfrozen epoch' % (len(moved) - sum(moved))
    net = vmods.resnext101_64x4d(num_classes=10).to(DEV).eval()
    with torch.no_grad():
        out = net(torch.randn(1, 3, 224, 224, device=DEV))
    assert out.shape == (1, 10) and torch.isfinite(out).all()
