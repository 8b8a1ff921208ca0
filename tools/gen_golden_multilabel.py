"""Golden vectors G18 for the multi-label image workflow (reference General/Learner.py:20,277-485, General/LossesMetrics.py:44-78,
Applications/Vision.py:1244-1337).

Runs the REAL reference on CPU through oracle/_ref_import.py (read-only; oracle/synth.py for closed-form parameters) and writes
data only to tests/golden/g18_multilabel.npz:
  (a) logits [5, 17] and 0/1 targets: nn.BCEWithLogitsLoss() value and input gradient, fbeta_loss(2, threshold=t) for t = 0.1 .. 0.5
      and fbeta_loss(2, use_thresh=False) on the rounded predictions;
  (b) ImageClassificationNet as G13b builds it (ResNet-34 body from retinanet.RetinaNet(., BasicBlock, [3, 4, 6, 3]), head
      [[512], [0., 0.]], fill_reference_init_), 17 categories, target_type 'multi_label': 10 Learner.train1minibatch steps at 64 x 64,
      bs 16, SGD momentum, wd 1e-4, on 10 DISTINCT learnable batches (`multilabel_batch`, regenerated from their tags by the tests) in
      fp32 and fp64.  Learning rates per layer group as G13b's docstring derives them: lr_g = GROUP_STEP / G_g^2 with G_g the group's
      gradient norm at the freshly initialised network (measured here on the first batch in fp64, rounded to one significant digit and
      stored), so that the groups are balanced; GROUP_STEP = 1e-2 as in G13b.  At bs 16 most of a batch's gradient fits that batch's
      noise, so over 10 distinct batches the curve falls by 0.03 only (0.918 -> 0.888); three times the rates (and twice the signal)
      fell no further and took the reference's own fp32 / fp64 runs 1.5e-4 apart, against 5e-6 here.  The generator asserts that the
      reference's own fp32 and fp64 curves stay within 3e-4 of each other and that the curve descends;
  (c) with the trained fp32 net: evaluate('val', metrics=[five f2]) and predict('val') on three fixed val minibatches (16, 16 and 7
      rows).  The val batches' tag is the one of 20 candidates whose sigmoids stay farthest from the thresholds 0.1 .. 0.5; the
      generator asserts that no sigmoid lies within 1e-4 of one and stores the margin (`c.margin`).
Usage: python tools/gen_golden_multilabel.py   (needs the reference checkout the oracle shim points at)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import synth  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g18_multilabel.npz')
SEP_LIMIT = 3e-4
GROUP_STEP = 1e-2         # lr_g G_g^2, the first-order loss change one step of one layer group causes
MARGIN = 1e-4
THRESHOLDS = [0.1, 0.2, 0.3, 0.4, 0.5]
NCAT, S, BS, STEPS = 17, 64, 16, 10
VAL_ROWS = [16, 16, 7]


def multilabel_targets(n, ncat, tag):
    "fixed 0/1 targets [n, ncat] fp32, about a third set (numpy legacy RandomState: bit-stable)"
    return torch.from_numpy((np.random.RandomState(500009 + int(tag)).random_sample((n, ncat)) < 0.35).astype(np.float32))


def multilabel_batch(n, size, ncat, tag, amp=0.5):
    """One LEARNABLE synthetic multi-label minibatch: 0.5 N(0, 1) noise [n, 3, size, size]; category j's 0/1 target is written as a
    +-amp offset into a band of rows of channel j % 3 (bands of size // ncat rows), so the curve descends."""
    x, y = synth.synth_input((n, 3, size, size), tag) * 0.5, multilabel_targets(n, ncat, tag)
    band = max(size // ncat, 1)
    for j in range(ncat):
        x[:, j % 3, band * j:band * (j + 1), :] += amp * (2.0 * y[:, j] - 1.0).view(-1, 1, 1)
    return x, y


def val_batches(tag):
    return [multilabel_batch(n, S, NCAT, 1850 + 10 * tag + k) for k, n in enumerate(VAL_ROWS)]


def threshold_margin(logits):
    "smallest distance of any sigmoid from any threshold (0.5, where predict() and the accuracy round, is one of them)"
    s = torch.as_tensor(logits).detach().double().sigmoid().reshape(-1, 1)
    return float((s - torch.tensor(THRESHOLDS, dtype=torch.float64).view(1, -1)).abs().min())


def A(t):
    return t.detach().cpu().numpy().copy()


def part_a(out, R):
    LM = R['General.LossesMetrics']
    x = synth.synth_input((5, NCAT), 1801, 2.0).requires_grad_(True)
    t = multilabel_targets(5, NCAT, 1802)
    assert threshold_margin(x) >= MARGIN
    loss = torch.nn.BCEWithLogitsLoss()(x, t)
    loss.backward()
    out.update({'a.logits': A(x), 'a.target': A(t), 'a.loss': A(loss), 'a.grad': A(x.grad), 'a.thresholds': np.array(THRESHOLDS)})
    with torch.no_grad():
        out['a.f2'] = np.array([LM.fbeta_loss(2, threshold=th)(x, t).item() for th in THRESHOLDS], dtype=np.float64)
        out['a.f2_rounded'] = np.array(LM.fbeta_loss(2, use_thresh=False)(x.sigmoid().round(), t).item(), dtype=np.float64)


class _D:
    sz, categories, bs, target_type = (S, S), {i: 'c%d' % i for i in range(NCAT)}, BS, 'multi_label'


def reference_net(R, dtype):
    RN, V = R['Applications.VisionModels.retinanet'], R['Applications.Vision']
    arch = RN.RetinaNet(2, RN.BasicBlock, [3, 4, 6, 3])
    net = V.ImageClassificationNet(_D, arch, head=[[512], [0., 0.]], cutpoint=8, splits=[6])
    synth.fill_reference_init_(net, seed=18)
    return net.to(dtype).train()


def group_lrs(R):
    "lr_g = GROUP_STEP / G_g^2 at the freshly initialised network (first batch, fp64), one significant digit"
    net = reference_net(R, torch.float64)
    x, y = multilabel_batch(BS, S, NCAT, 1810)
    torch.nn.BCEWithLogitsLoss()(net(x.double()), y.double()).backward()
    lrs, norms = [], []
    for group in net.layer_groups:
        g = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in group.parameters() if p.grad is not None)))
        norms.append(g)
        lrs.append(float('%.0e' % (GROUP_STEP / g ** 2)))
    print('gradient norms per layer group', norms, '-> lr', lrs, flush=True)
    return lrs, norms


def part_bc(out, R):
    Learner, LM = R['General.Learner'].Learner, R['General.LossesMetrics']
    lr, norms = group_lrs(R)
    out.update({'b.N': BS, 'b.S': S, 'b.ncat': NCAT, 'b.steps': STEPS, 'b.lr': np.array(lr), 'b.group_grad_norms': np.array(norms),
                'b.wd': 1e-4, 'b.init_seed': 18, 'b.tag0': 1810})
    for tag, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        net = reference_net(R, dtype)
        d = _D(); d.train_dl = [(None, torch.zeros(BS))]; d.val_dl = d.train_dl
        learner = Learner('/tmp/nnl_golden_g18', d, net, optimizer='SGD_Mom')
        assert type(learner.loss_func) is torch.nn.BCEWithLogitsLoss
        learner.init_optimizer(wd=1e-4)
        losses = []
        for i in range(STEPS):
            x, y = multilabel_batch(BS, S, NCAT, 1810 + i)
            losses.append(learner.train1minibatch(x.to(dtype), y.to(dtype), lr))
            print(tag, i, losses[-1], flush=True)
        out['b.losses.' + tag] = np.array(losses, dtype=np.float64)
        if tag == 'f32':
            out['b.param_names'] = np.array([n for n, _ in net.named_parameters()])
            trained = learner
    l32, l64 = out['b.losses.f32'], out['b.losses.f64']
    sep = np.abs(l32 - l64) / np.abs(l64)
    print('g18(b) fp32-vs-fp64 relative separation per step:', np.array2string(sep, precision=1), flush=True)
    assert sep.max() < SEP_LIMIT, 'g18(b): the reference itself separates by %.1e: fixture not well conditioned' % sep.max()
    assert l32[-1] < l32[0] - 5e-3, 'g18(b): the curve does not descend (%r)' % (l32,)

    # (c) the trained fp32 net in eval mode
    net = trained.model
    net.eval()
    best = None
    with torch.no_grad():
        for cand in range(20):
            m = threshold_margin(torch.cat([net(x) for x, _ in val_batches(cand)]))
            if best is None or m > best[0]:
                best = (m, cand)
    margin, cand = best
    print('g18(c) val tag %d: smallest |sigmoid - threshold| = %.2e' % (cand, margin), flush=True)
    assert margin >= MARGIN, 'g18(c): a val sigmoid lies within %.0e of a threshold' % MARGIN
    trained.data.val_dl = val_batches(cand)
    metrics = [LM.fbeta_loss(2, threshold=th) for th in THRESHOLDS]
    res = trained.evaluate('val', metrics=metrics)
    probs, labels = trained.predict('val')
    out.update({'c.val_tag': cand, 'c.margin': margin, 'c.rows': np.array(VAL_ROWS), 'c.loss': np.array(res[0], dtype=np.float64),
                'c.accuracy': np.array(res[1], dtype=np.float64), 'c.metrics': np.asarray(res[2], dtype=np.float64),
                'c.probs': probs.astype(np.float32), 'c.labels': labels.astype(np.int8)})
    print('g18(c) loss %.6f accuracy %.6f f2 %s' % (res[0], res[1], np.array2string(np.asarray(res[2]), precision=4)), flush=True)


def main():
    from oracle import _ref_import
    R = _ref_import.load()
    out = {}
    part_a(out, R)
    part_bc(out, R)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, '%.1f KB' % (os.path.getsize(OUT) / 1024))


if __name__ == '__main__':
    main()
