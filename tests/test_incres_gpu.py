"""InceptionResNetV2 on the GPU against golden G30 (tools/gen_golden_incres.py: the real reference on CPU in fp32 and fp64).

The rule of tests/test_nasnet_gpu.py, with the margin tests/test_inception_gpu.py uses: |hip - f64| <= 3 |ref32 - f64| + 1e-3 |f64| — per
tensor in max-norm for activations, input gradients and running statistics (of a large activation the channels the golden file holds:
`held`), per value for losses, gradient sums and the curve; figures are printed before they are asserted.  The full 43-block class only
runs: one forward and one training step at 75 x 75, the smallest image that leaves a 1 x 1 map, with every gradient finite."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_inception_gpu import grad_sums, learner_for
from test_nasnet_gpu import bn_stats, rule
from tools.gen_golden_incres import block_cases, held, short_net
from tools.gen_golden_inception import CURVE_LR, FEATURES, STEPS, batch, block_input, block_weight, build

from neuralnetworklibrary_amd.Applications.VisionModels import inceptionresnetv2, vmods

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BLOCKS = list(block_cases(inceptionresnetv2))

g30 = pytest.fixture(scope='module')(lambda: load_golden('g30_incres'))


def stats_rule(g, key, net):
    for what, got in zip(('rmean', 'rvar'), bn_stats(net)):
        rule('%s %s' % (key, what), got, g['%s.%s.f64' % (key, what)], dev32=g['%s.%s.dev32' % (key, what)])


@pytest.mark.parametrize('name', BLOCKS)
def test_each_block_alone_follows_the_reference(g30, name):
    index = BLOCKS.index(name)
    make, shape = block_cases(inceptionresnetv2)[name]
    block = build(make).to(DEV).train()
    x = block_input(shape, index).to(DEV).requires_grad_(True)
    y = block(x)
    (y * block_weight(y.shape, index).to(DEV)).sum().backward()
    key = 'block.' + name
    rule(key + ' out', held(y), g30[key + '.out.f64'], dev32=g30[key + '.out.dev32'])
    rule(key + ' din', held(x.grad), g30[key + '.din.f64'], dev32=g30[key + '.din.dev32'])
    rule(key + ' grad sums', grad_sums(block), g30[key + '.gsum.f64'], r32=g30[key + '.gsum.f32'])
    stats_rule(g30, key, block)


def test_short_network_eval_train_and_curve_follow_the_reference(g30, tmp_path):
    make = short_net(inceptionresnetv2)
    x, y = (t.to(DEV) for t in batch())
    net = build(make).to(DEV).eval()
    with torch.no_grad():
        feat = net.features(x)
    assert feat.shape == (4, FEATURES, 2, 2)
    rule('short features', held(feat), g30['short.feat.f64'], dev32=g30['short.feat.dev32'])
    net = build(make).to(DEV).train()
    loss = F.cross_entropy(net(x), y)
    loss.backward()
    rule('short loss', loss.item(), g30['short.loss.f64'], r32=g30['short.loss.f32'])
    rule('short grad sums', grad_sums(net), g30['short.gsum.f64'], r32=g30['short.gsum.f32'])
    stats_rule(g30, 'short', net)
    learner = learner_for(build(make), tmp_path)
    curve = [learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(STEPS)]
    rule('short curve', curve, g30['short.curve.f64'], r32=g30['short.curve.f32'])


def test_short_network_graph_replay_is_bit_equal_to_eager(tmp_path):
    x, y = (t.to(DEV) for t in batch())
    runs = []
    for graphs in (False, True):
        learner = learner_for(build(short_net(inceptionresnetv2)), tmp_path)
        if graphs:
            learner.use_graphs(warmup=2)
        losses = [learner.train1minibatch(x, y, [CURVE_LR]) for _ in range(5)]
        if graphs:
            assert len(learner._graphs) == 1 and next(iter(learner._graphs.values())).graph is not None
        runs.append((losses, [p.detach().clone() for p in learner.model.parameters()]))
    (le, pe), (lg, pg) = runs
    assert le == lg
    assert all(torch.equal(a, b) for a, b in zip(pe, pg))


def test_full_class_runs_forward_and_one_training_step():
    x, y = torch.randn(2, 3, 75, 75, generator=torch.Generator().manual_seed(0)).to(DEV), torch.tensor([1, 3], device=DEV)
    net = build(lambda: vmods.inceptionresnetv2(num_classes=5)).to(DEV).train()
    feat = net(x)
    assert feat.shape == (2, 1536, 1, 1) and bool(torch.isfinite(feat).all())
    with torch.no_grad():
        assert net.eval()(x, use_logits=True).shape == (2, 5)
    logits = net.train()(x, use_logits=True)
    F.cross_entropy(logits, y).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    opt.step()
    assert bool(torch.isfinite(net(x, use_logits=True)).all())
