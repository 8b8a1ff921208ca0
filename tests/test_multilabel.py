"""The multi-label image workflow (the Planet notebook): nn.BCEWithLogitsLoss() and fbeta_loss on the HIP kernels of csrc/loss.hip,
ImageBatches.with_transform, ImageLearner.data_resize / switch_transform_stats / confusion_matrix / TTA, and golden G18
(tools/gen_golden_multilabel.py: the real reference's loss, metric, 10-step curve at 64 x 64 and evaluate / predict)."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import assert_close, load_golden
from oracle import synth
from tools.gen_golden_multilabel import multilabel_batch, threshold_margin, val_batches

from neuralnetworklibrary_amd import device_data, ops
from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.General.Learner import HipBCEWithLogitsLoss, Learner, loss_func_dict
from neuralnetworklibrary_amd.General.LossesMetrics import fbeta_loss

DEV = 'cuda'
THRESHOLDS = [0.1, 0.2, 0.3, 0.4, 0.5]
ONE_BLOCK = 65536            # csrc/loss.hip kLossOneBlock: one 1024-thread block up to here, partials + a final kernel above


def torch_fbeta(y_pred, y_true, beta, threshold=0.5, use_thresh=True, eps=1e-9):
    "the plain torch expression of fbeta_loss.__call__ (reference General/LossesMetrics.py:70-78)"
    b2 = beta ** 2
    y_pred = (y_pred.sigmoid() >= threshold).float() if use_thresh else y_pred.float()
    y_true = y_true.float()
    tp = (y_pred * y_true).sum(dim=1)
    p = tp / (y_pred.sum(dim=1) + eps)
    r = tp / (y_true.sum(dim=1) + eps)
    return torch.mean((1 + b2) * (p * r) / (b2 * p + r + eps))


# ---- CPU: the torch paths, the registry, the bookkeeping ----------------------------------------------------------------------

def test_cpu_loss_and_metric_are_torch_bit_for_bit_and_match_g18a():
    g = load_golden('g18_multilabel')
    x, t = torch.from_numpy(g['a.logits']).requires_grad_(True), torch.from_numpy(g['a.target'])
    assert tuple(x.shape) == (5, 17) and set(np.unique(g['a.target'])) <= {0.0, 1.0}
    loss = HipBCEWithLogitsLoss()(x, t)
    loss.backward()
    assert torch.equal(loss, F.binary_cross_entropy_with_logits(x.detach(), t))
    assert_close(loss, g['a.loss'], 1e-6, 0, 'G18(a) loss')
    assert_close(x.grad, g['a.grad'], 1e-6, 1e-9, 'G18(a) d logits')
    for th, want in zip(THRESHOLDS, g['a.f2']):
        got = fbeta_loss(2, threshold=th)(x.detach(), t)
        assert torch.equal(got, torch_fbeta(x.detach(), t, 2, th))
        assert_close(got, want, 1e-6, 0, 'G18(a) f2 at %.1f' % th)
    rounded = x.detach().sigmoid().round()
    got = fbeta_loss(2, use_thresh=False)(rounded, t)
    assert torch.equal(got, torch_fbeta(rounded, t, 2, use_thresh=False))
    assert_close(got, g['a.f2_rounded'], 1e-6, 0, 'G18(a) f2 of rounded predictions')


def test_multi_label_default_loss_is_a_bce_with_logits_loss():
    lf = loss_func_dict['multi_label']
    assert isinstance(lf, nn.BCEWithLogitsLoss) and isinstance(lf, HipBCEWithLogitsLoss)
    assert lf.weight is None and lf.pos_weight is None and lf.reduction == 'mean'
    assert V.HipBCEWithLogitsLoss is HipBCEWithLogitsLoss


def test_new_ops_refuse_cpu_tensors_and_c_entries_report_bad_arguments():
    from neuralnetworklibrary_amd._lib import NnlError, lib
    a = torch.zeros(3, 4)
    with pytest.raises(NnlError):
        ops.bce_with_logits(a, a)
    with pytest.raises(NnlError):
        ops.fbeta(a, a, 2)
    assert lib.nnl_bce_logits_fwd(None, None, None, 4, None, 0, None) == -1 and b'bce_logits_fwd' in lib.nnl_last_error()
    assert lib.nnl_bce_logits_bwd(None, None, None, None, 4, None) == -1 and b'bce_logits_bwd' in lib.nnl_last_error()
    assert lib.nnl_fbeta(None, None, None, 4, 4, 4., .5, 1, 1e-9, None, 0, None) == -1 and b'fbeta' in lib.nnl_last_error()
    assert lib.nnl_bce_logits_workspace_bytes(ONE_BLOCK) == 0 and lib.nnl_bce_logits_workspace_bytes(ONE_BLOCK + 1) > 0
    assert lib.nnl_fbeta_workspace_bytes(4096, 17) == 0 and lib.nnl_fbeta_workspace_bytes(4097, 17) > 0


SHAPES = [(13, 17), (17, 13), (16, 16), (9, 31), (40, 23), (5, 7), (8, 8)]


def _images(seed, target):
    rs = np.random.RandomState(seed)
    return [{'img': rs.randint(0, 256, (H, W, 3)).astype(np.uint8), 'target': target(i)} for i, (H, W) in enumerate(SHAPES)]


@pytest.fixture
def stub_kernel(monkeypatch):
    "ops.image_aug replaced by a recorder of the parameter rows of every call; zeros out"
    calls = []

    def fake(arena, desc, params, sz, stats=None, lighting=False):
        rows = params.cpu().numpy().view(ops.IMAGE_AUG_PARAM).reshape(-1).copy()
        calls.append((rows, tuple(sz), stats))
        return torch.zeros(len(rows), sz[0], sz[1], 3)
    monkeypatch.setattr(ops, 'image_aug', fake)
    return calls


def _stub_learner(target_type='multi_label', tfm_type='TopDown', sz=8, test=True):
    "an ImageLearner over host-resident stub loaders, without a model: what data_resize / switch_transform_stats / TTA touch"
    tfm_eval, tfm_aug = V.get_transforms(tfm_type, sz)
    target = (lambda i: np.array([i % 2, 1, 0])) if target_type == 'multi_label' else (lambda i: i % 3)
    d = types.SimpleNamespace(target_type=target_type, categories={0: 'a', 1: 'b', 2: 'c'}, bs=3, sz=tfm_eval.sz)
    d.train_ds = V.ImageDataset('', _images(1, target), tfm_aug, target_type, 'train')
    d.val_ds = V.ImageDataset('', _images(2, target), tfm_eval, target_type, 'val')
    d.test_ds = V.ImageDataset('', _images(3, lambda i: 0), tfm_eval, target_type, 'test') if test else None
    d.train_dl = device_data.ImageBatches(d.train_ds, 3, shuffle=True, seed=5, rank=1, world=2, device='cpu')
    d.val_dl = device_data.ImageBatches(d.val_ds, 3, shuffle=False, seed=5, device='cpu')
    d.test_dl = device_data.ImageBatches(d.test_ds, 3, shuffle=False, seed=5, device='cpu') if test else None
    learner = object.__new__(V.ImageLearner)
    learner.data, learner.target_type, learner._graphs = d, target_type, {'a captured step': None}
    return learner


def test_with_transform_shares_the_arena_and_draws_its_own(stub_kernel):
    learner = _stub_learner()
    val = learner.data.val_dl
    tfm = V.Transform('TopDown', 0.33, None, 12, 5, 1.0)
    view = val.with_transform(tfm, bs=4, seed=9)
    assert view is not val and view.arena.data_ptr() == val.arena.data_ptr() and view.desc.data_ptr() == val.desc.data_ptr()
    assert view.y.data_ptr() == val.y.data_ptr() and view.transform is tfm and val.transform is learner.data.val_ds.transform
    assert (view.bs, view.seed, view.shuffle, view.rank, view.world, view.epoch) == (4, 9, False, 0, 1, 0) and (val.bs, val.seed) == (3, 5)
    assert len(view) == 2 and len(val) == 3
    batches = list(view)
    assert [tuple(x.shape) for x, _ in batches] == [(4, 3, 12, 12), (3, 3, 12, 12)]
    assert torch.equal(torch.cat([y for _, y in batches]), val.y)
    rs = np.random.RandomState(9)
    want = [tfm.param_row(i, H, W, **tfm.sample(rs, H, W)) for i, (H, W) in enumerate(SHAPES)]
    assert np.array_equal(np.concatenate([rows for rows, _, _ in stub_kernel]), np.stack(want))
    same = val.with_transform(tfm)                               # defaults: the loader's own batch size and seed
    assert (same.bs, same.seed, same.shuffle) == (3, 5, False)
    sharded = learner.data.train_dl.with_transform(tfm)          # a view is rank-local and covers the full set
    assert (sharded.rank, sharded.world) == (0, 1) and len(sharded) == 3


def test_data_resize_bookkeeping(stub_kernel):
    learner = _stub_learner()
    d = learner.data
    tfms = [d.train_ds.transform, d.val_ds.transform, d.test_ds.transform]
    loaders = [d.train_dl, d.val_dl, d.test_dl]
    list(d.train_dl)                                             # one epoch drawn: the resized loader goes on with the next permutation
    learner.data_resize(16)
    assert d.sz == (16, 16) and all(t.sz == (16, 16) for t in tfms) and learner._graphs == {}
    assert [d.train_dl, d.val_dl, d.test_dl] == loaders and d.bs == 3          # no bs: the same loaders
    assert d.train_ds.transform is tfms[0] and d.train_dl.transform is tfms[0] and d.val_dl.transform is tfms[1]
    assert tuple(next(iter(d.val_dl))[0].shape) == (3, 3, 16, 16)
    learner._graphs = {'again': None}
    learner.data_resize((12, 12), bs=2)
    assert d.sz == (12, 12) and all(t.sz == (12, 12) for t in tfms) and d.bs == 2 and learner._graphs == {}
    for new, old in zip([d.train_dl, d.val_dl, d.test_dl], loaders):
        assert new is not old and new.bs == 2 and new.arena.data_ptr() == old.arena.data_ptr() and new.transform is old.transform
    assert d.train_dl.shuffle and (d.train_dl.rank, d.train_dl.world, d.train_dl.seed) == (1, 2, 5) and d.train_dl.epoch == 1
    assert not d.val_dl.shuffle and (d.val_dl.rank, d.val_dl.world) == (0, 1) and len(d.val_dl) == 4 and len(d.train_dl) == 2
    assert d.train_dl.transform is d.train_ds.transform and d.test_dl.transform is d.test_ds.transform
    x, y = next(iter(d.train_dl))
    assert tuple(x.shape) == (2, 3, 12, 12) and d.train_dl.dp_info == (2, 4)         # rank 1 of 2: its half of the first global minibatch of 4
    with pytest.raises(ValueError, match='TopDown'):
        learner.data_resize((12, 16))
    assert d.sz == (12, 12) and all(t.sz == (12, 12) for t in tfms)                   # refused before anything changed
    side = _stub_learner(tfm_type='SideOn', test=False)
    side.data_resize((12, 16), bs=4)
    assert side.data.sz == (12, 16) and side.data.val_ds.transform.sz == (12, 16) and side.data.test_dl is None
    assert tuple(next(iter(side.data.val_dl))[0].shape) == (4, 3, 12, 16)
    bbox = _stub_learner()
    bbox.data.target_type = 'bbox'
    with pytest.raises(ValueError, match='bbox'):
        bbox.data_resize(16)


def test_switch_transform_stats(stub_kernel):
    learner = _stub_learner()
    d = learner.data
    learner.switch_transform_stats(V.alternate_stats)
    assert all(t.stats is V.alternate_stats for t in (d.train_ds.transform, d.val_ds.transform, d.test_ds.transform))
    next(iter(d.val_dl))
    assert stub_kernel[-1][2] is V.alternate_stats               # the loaders read the shared Transform objects
    _stub_learner(test=False).switch_transform_stats(V.alternate_stats)


def test_tta_transforms_views_and_weights_are_the_reference_list(stub_kernel):
    """reference Vision.py:2014-2033: tfm0 = Transform('Basic','center',None,sz,None,None,None,None,stats=stats), tfm1..4 =
    Transform(tfm_type, c, None, sz, 5, 1.0, stats=stats) for c = 0.0, 0.33, 0.67, 1.0 with the TRAIN transform's type, stats and
    size; weights [beta, (1 - beta) / 4 x 4]; bs = data.bs; predictions through self.predict(loader)[0]"""
    learner = _stub_learner()
    d = learner.data
    d.train_ds.transform.stats = V.alternate_stats                # only the train transform's stats count
    d.bs = 4
    tfms, weights = learner.tta_transforms(0.4)
    attrs = lambda t: (t.tfm_type, t.crop_type, t.pad, t.sz, t.max_deg, t.max_zoom, t.bal_range, t.cont_range, t.max_noise)
    assert attrs(tfms[0]) == ('Basic', 'center', None, (8, 8), None, None, None, None, None)
    for t, c in zip(tfms[1:], (0.0, 0.33, 0.67, 1.0)):
        assert attrs(t) == ('TopDown', c, None, (8, 8), 5, 1.0, [-0.05, 0.05], [0.95, 1.05], None) and type(t.crop_type) == float
    assert len(tfms) == 5 and all(t.stats is V.alternate_stats for t in tfms)
    assert weights == [0.4, (1 - 0.4) / 4, (1 - 0.4) / 4, (1 - 0.4) / 4, (1 - 0.4) / 4]
    seen = []

    def predict(dl):
        seen.append(dl)
        k = len(seen)
        return [np.full((7, 3), 0.1 * k), None]
    learner.predict = predict
    for ds_type, base in (('val', d.val_dl), ('test', d.test_dl)):
        del seen[:]
        probs, labels = learner.TTA(ds_type, beta=0.2)
        assert [v.seed for v in seen] == [5, 6, 7, 8, 9] and all(v.bs == 4 and not v.shuffle for v in seen)
        assert all(v.arena.data_ptr() == base.arena.data_ptr() and v is not base for v in seen)
        assert [attrs(v.transform) for v in seen] == [attrs(t) for t in tfms]
        want = V.combine_preds([np.full((7, 3), 0.1 * k) for k in range(1, 6)], 'multi_label', [0.2, 0.2, 0.2, 0.2, 0.2])
        assert np.array_equal(probs, want[0]) and np.array_equal(labels, want[1])
    learner.target_type = 'cont'
    with pytest.raises(ValueError):
        learner.TTA('val')
    learner.target_type = 'multi_label'
    with pytest.raises(ValueError):
        learner.TTA('train')
    with pytest.raises(ValueError, match='single_label'):
        learner.confusion_matrix()


# ---- GPU: the kernels --------------------------------------------------------------------------------------------------------

def _bce_inputs(n, seed):
    "logits ~ 3 N(0, 1) and SOFT targets ~ U[0, 1]; from 51 elements on, logits of +-100 against targets 0, 1 and in between"
    g = torch.Generator().manual_seed(seed)
    x, t = torch.randn(n, generator=g) * 3, torch.rand(n, generator=g)
    if n >= 51:
        x[:4] = torch.tensor([100., -100., 100., -100.])
        t[:4] = torch.tensor([0., 1., 0.25, 0.75])
    return x, t


def _check_bce(x, t, xd, td, lf):
    "value and d logits of lf(xd, td) under an upstream gradient of 2.5 against torch fp64 on the CPU"
    x64 = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(x64, t.double())
    (2.5 * ref).backward()
    xd = xd.requires_grad_(True)
    out = lf(xd, td)
    (2.5 * out).backward()
    assert out.dtype == torch.float32 and out.dim() == 0 and torch.isfinite(out) and torch.isfinite(xd.grad).all()
    assert xd.grad.shape == xd.shape
    grad = xd.grad.reshape(-1)
    err = (grad.cpu().double() - x64.grad).abs().max().item()
    print('n %d: loss %.9g (fp64 %.9g), max |d logits err| %.3e of max |d logits| %.3e' % (
        x.numel(), out.item(), ref.item(), err, x64.grad.abs().max().item()))
    assert_close(out.reshape(1), np.array([float(ref.detach())]), 2e-6, 1e-7, 'value')
    assert_close(grad, x64.grad.float(), 1e-6, 1e-7 * float(x64.grad.abs().max()), 'd logits')
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 51, 1088, ONE_BLOCK, ONE_BLOCK + 1])
def test_hip_bce_with_logits_vs_torch_fp64(n, monkeypatch):
    """nn.BCEWithLogitsLoss() of the 'multi_label' target type (reference General/Learner.py:20) on the HIP kernels: value and d logits
    against torch in fp64 with an upstream gradient of 2.5 (the tolerances of test_hip_mse_loss_vs_torch), soft targets, logits of +-100,
    sizes that are no multiple of 4 and on both sides of the one-block limit, and bitwise reproducibility of the fixed-order sum."""
    calls = []
    real = ops.bce_with_logits
    monkeypatch.setattr(ops, 'bce_with_logits', lambda a, b: (calls.append(1), real(a, b))[1])
    x, t = _bce_inputs(n, n)
    shape = (n // 17, 17) if n % 17 == 0 else (n,)
    _check_bce(x, t, x.to(DEV).view(shape), t.to(DEV).view(shape), loss_func_dict['multi_label'])
    assert calls == [1]                                          # the HIP path, not torch's
    assert torch.equal(real(x.to(DEV), t.to(DEV)), real(x.to(DEV), t.to(DEV)))


@pytest.mark.gpu
def test_hip_bce_with_logits_unaligned_pointers_and_torch_path(monkeypatch):
    """logits that start 4 bytes past a 16-byte boundary (a sliced view of a larger buffer is contiguous, so the op hands the kernel
    that pointer: the backward then takes its scalar path), then with aligned logits and an offset target; and a loss with
    pos_weight, which is torch's own"""
    n = 1088
    x, t = _bce_inputs(n, 7)
    lf = HipBCEWithLogitsLoss()
    base = torch.zeros(n + 1, device=DEV)
    base[1:] = x.to(DEV)
    xd = base[1:].detach()
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    a = _check_bce(x, t, xd, t.to(DEV), lf)
    tbase = torch.zeros(n + 3, device=DEV)
    tbase[3:] = t.to(DEV)
    assert tbase[3:].data_ptr() % 16 == 12
    b = _check_bce(x, t, x.to(DEV), tbase[3:], lf)
    assert torch.equal(a, b)                                     # the forward does not depend on the alignment
    monkeypatch.setattr(ops, 'bce_with_logits', lambda a, b: pytest.fail('a loss with pos_weight took the HIP path'))
    pw = torch.linspace(0.5, 2.0, 17, device=DEV)
    x2, t2 = x.to(DEV).view(64, 17), t.to(DEV).view(64, 17)
    assert torch.equal(HipBCEWithLogitsLoss(pos_weight=pw)(x2, t2), F.binary_cross_entropy_with_logits(x2, t2, pos_weight=pw))
    assert torch.equal(HipBCEWithLogitsLoss(reduction='sum')(x2, t2), F.binary_cross_entropy_with_logits(x2, t2, reduction='sum'))


def _fbeta_inputs(N, C, seed):
    """logits ~ 2 N(0, 1) moved off the thresholds, 0/1 targets; from 3 rows on: row 0 predicts nothing (logits -10) and has a positive
    target, row 1 has no positive target, row 2 is both; unless that is the last row, the last row's first logit is EXACTLY 0
    (sigmoid 0.5: `>=` counts it at threshold 0.5) with target 1"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g) * 2
    t = (torch.rand(N, C, generator=g) < 0.4).float()
    for _ in range(4):
        near = ((x.double().sigmoid().unsqueeze(-1) - torch.tensor(THRESHOLDS, dtype=torch.float64)).abs() < 1e-3).any(-1)
        x = torch.where(near, x + 0.05, x)
    if N >= 3:
        x[0], t[0, 0], t[1] = -10., 1., 0.
        x[2], t[2] = -10., 0.
    if N != 3:
        x[N - 1, 0], t[N - 1, 0] = 0., 1.
    return x, t


@pytest.mark.gpu
@pytest.mark.parametrize('N,C', [(1, 1), (3, 17), (64, 17), (5, 130), (4097, 3)])
def test_hip_fbeta_vs_torch(N, C):
    """fbeta_loss.__call__ in one launch against the torch expression on the CPU: beta 2, the notebook's five thresholds and
    use_thresh=False on rounded predictions; rows without a positive prediction, without a positive target and without both (eps
    1e-9 gives the zeros torch gives); a logit of exactly 0 at threshold 0.5; C above a wavefront; N above the one-block row limit."""
    x, t = _fbeta_inputs(N, C, 100 * N + C)
    s = x.double().sigmoid()
    exact0 = x == 0
    for th in THRESHOLDS:
        far = (s - th).abs() >= 1e-4
        assert (far | (exact0 if th == 0.5 else torch.zeros_like(exact0))).all()
    assert exact0.any() == (N != 3) and (N < 3 or ((x.sigmoid() >= 0.1).sum(1)[0] == 0 and t[1].sum() == 0 and t[0].sum() > 0))
    xd, td = x.to(DEV), t.to(DEV)
    for th in THRESHOLDS:
        got, want = fbeta_loss(2, threshold=th)(xd, td), torch_fbeta(x, t, 2, th)
        assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 0
        print('(%d, %d) threshold %.1f: %.9g (torch %.9g)' % (N, C, th, got.item(), want.item()))
        assert_close(got, want, 2e-6, 1e-7, 'f2 at threshold %.1f' % th)
        assert torch.equal(got, ops.fbeta(xd, td, 2, th))
    rounded = x.sigmoid().round()
    assert_close(fbeta_loss(2, use_thresh=False)(rounded.to(DEV), td), torch_fbeta(rounded, t, 2, use_thresh=False), 2e-6, 1e-7, 'rounded')
    if N >= 3:                                                   # the three degenerate rows alone score exactly 0, as in torch
        assert fbeta_loss(2, threshold=0.5)(xd[:3], td[:3]).item() == torch_fbeta(x[:3], t[:3], 2, 0.5).item() == 0.0
    if N != 3:                                                   # the exact 0 counts as predicted: that 1 x 1 problem scores 1, not 0
        assert fbeta_loss(2, threshold=0.5)(xd[N - 1:, :1], td[N - 1:, :1]).item() == pytest.approx(1.0, abs=1e-6)
    # anything but same-shape CUDA fp32 [N, C] takes the torch expression
    assert_close(fbeta_loss(2, threshold=0.3)(xd.double(), td.double()), torch_fbeta(x.double(), t.double(), 2, 0.3), 1e-6, 1e-7, 'fp64 inputs')


@pytest.mark.gpu
def test_g18a_loss_gradient_and_metric_on_the_kernels():
    """G18(a): the reference's own fp32 values.  Both sides round in fp32, so the gradient's absolute term is 3e-7 of the largest
    gradient (each side's sigmoid is within ~1.5 ulp(1) = 9e-8) where the fp64 comparison above has 1e-7."""
    g = load_golden('g18_multilabel')
    x, t = torch.from_numpy(g['a.logits']).to(DEV).requires_grad_(True), torch.from_numpy(g['a.target']).to(DEV)
    loss = loss_func_dict['multi_label'](x, t)
    loss.backward()
    assert_close(loss, g['a.loss'], 2e-6, 1e-7, 'G18(a) loss')
    assert_close(x.grad, g['a.grad'], 1e-6, 3e-7 * float(np.abs(g['a.grad']).max()), 'G18(a) d logits')
    for th, want in zip(THRESHOLDS, g['a.f2']):
        assert_close(fbeta_loss(2, threshold=th)(x.detach(), t), want, 2e-6, 1e-7, 'G18(a) f2 at %.1f' % th)
    assert_close(fbeta_loss(2, use_thresh=False)(x.detach().sigmoid().round(), t), g['a.f2_rounded'], 2e-6, 1e-7, 'G18(a) rounded')


# ---- GPU: G18(b), (c) — the reference's 10-step curve at 64 x 64 and its evaluate / predict ---------------------------------------

def _g18_learner(g):
    N, S, ncat = int(g['b.N']), int(g['b.S']), int(g['b.ncat'])

    class D:
        sz, categories, bs, target_type = (S, S), {i: 'c%d' % i for i in range(ncat)}, N, 'multi_label'
    net = V.ImageClassificationNet(D, V.models.resnet34(), head=[[512], [0., 0.]])
    synth.fill_reference_init_(net, seed=int(g['b.init_seed']))
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in g['b.param_names']]
    d = D(); d.train_dl = [(None, torch.zeros(N))]; d.val_dl = d.train_dl
    learner = Learner('/tmp/nnl_test_g18', d, net.to(DEV), optimizer='SGD_Mom')
    assert learner.loss_func is loss_func_dict['multi_label']
    learner.init_optimizer(wd=float(g['b.wd']))
    net.train()
    return learner


def _g18_curve(g, learner):
    N, S, ncat, lr = int(g['b.N']), int(g['b.S']), int(g['b.ncat']), [float(v) for v in g['b.lr']]
    losses = []
    for i in range(int(g['b.steps'])):
        x, y = multilabel_batch(N, S, ncat, int(g['b.tag0']) + i)
        losses.append(learner.train1minibatch(x.to(DEV), y.to(DEV), lr))
    return np.array(losses)


@pytest.fixture(scope='module')
def g18_eager():
    g = load_golden('g18_multilabel')
    learner = _g18_learner(g)
    return g, learner, _g18_curve(g, learner)


def _check_curve(g, losses, what):
    r32, r64 = g['b.losses.f32'], g['b.losses.f64']
    assert (np.abs(r32 - r64) / np.abs(r64)).max() < 3e-4                     # the fixture is well conditioned
    rel = np.abs(losses - r32) / np.abs(r32)
    print(what, 'losses', np.array2string(losses, precision=5))
    print(what, 'rel |hip - ref32|', np.array2string(rel, precision=1), ' rel |ref32 - ref64|', np.array2string(np.abs(r32 - r64) / np.abs(r64), precision=1))
    assert (rel <= 1e-3).all(), '%s: step losses off the reference fp32 curve: worst %.2e at step %d' % (what, rel.max(), rel.argmax())


@pytest.mark.gpu
def test_g18b_multilabel_10_step_curve_at_64px_within_1e3(g18_eager):
    """10 `Learner.train1minibatch` steps of ResNet-34 + head, 17 categories, at 64 x 64 (a 2 x 2 last stage), bs 16, with the default
    multi-label loss, against the REFERENCE's own Learner: every step within 1e-3 relative of its fp32 curve (the project's parity
    contract, as for G13b)."""
    g, _, losses = g18_eager
    _check_curve(g, losses, 'eager')


@pytest.mark.gpu
def test_g18b_curve_under_graph_replay(g18_eager):
    "the same curve with use_graphs(warmup=2): within 1e-3 of the reference, and the replayed losses equal the eager ones of this build"
    g, _, eager = g18_eager
    learner = _g18_learner(g).use_graphs(warmup=2)
    losses = _g18_curve(g, learner)
    step = next(iter(learner._graphs.values()))
    assert len(learner._graphs) == 1 and step.graph is not None                # steps 3 .. 10 were replays
    _check_curve(g, losses, 'replayed')
    assert_close(losses, eager, 1e-5, 1e-6, 'losses: graph replay vs eager')


@pytest.mark.gpu
def test_g18c_evaluate_and_predict_match_the_reference(g18_eager):
    """evaluate('val', metrics=[five f2]) and predict('val') of the trained net on three val minibatches (16, 16, 7 rows): loss,
    multi-label accuracy and metrics within 1e-3 relative, probabilities within 1e-3 absolute, labels identical (the generator kept
    every sigmoid at least 1e-4 from the thresholds)."""
    g, learner, _ = g18_eager
    assert float(g['c.margin']) >= 1e-4 and [int(n) for n in g['c.rows']] == [16, 16, 7]
    learner.data.val_dl = [(x.to(DEV), y.to(DEV)) for x, y in val_batches(int(g['c.val_tag']))]
    res = learner.evaluate('val', metrics=[fbeta_loss(2, threshold=th) for th in THRESHOLDS])
    probs, labels = learner.predict('val')
    print('loss %.6f (ref %.6f) accuracy %.6f (ref %.6f)' % (res[0], g['c.loss'], res[1], g['c.accuracy']))
    print('f2', np.array2string(np.asarray(res[2]), precision=6), 'ref', np.array2string(g['c.metrics'], precision=6))
    print('max |probs - ref| %.2e, margin of the probabilities %.2e' % (np.abs(probs - g['c.probs']).max(), threshold_margin(torch.from_numpy(probs).logit())))
    assert_close(np.array(res[0]), g['c.loss'], 1e-3, 0, 'val loss')
    assert_close(np.array(res[1]), g['c.accuracy'], 1e-3, 0, 'multi-label accuracy')
    assert_close(np.asarray(res[2]), g['c.metrics'], 1e-3, 0, 'f2 metrics')
    assert probs.shape == (39, 17) and labels.shape == (39, 17)
    assert_close(probs, g['c.probs'], 0, 1e-3, 'probabilities')
    assert np.array_equal(labels, g['c.labels'].astype(labels.dtype))


# ---- GPU: the notebook's call sequence from the public API -------------------------------------------------------------------------

def _decoded(n, seed, target):
    rs = np.random.RandomState(seed)
    return [{'img': rs.randint(0, 256, (rs.randint(33, 48), rs.randint(33, 48), 3)).astype(np.uint8), 'target': target(rs, i)} for i in range(n)]


@pytest.fixture
def quiet():
    verbose, Learner.verbose = Learner.verbose, False
    yield
    Learner.verbose = verbose


@pytest.mark.gpu
def test_planet_workflow_end_to_end(tmp_path, quiet):
    "freeze / bn_freeze / fit with an F2 metric / unfreeze / bn_unfreeze / use_graphs / fit / data_resize / fit / TTA, multi-label"
    multi = lambda rs, i: (rs.random_sample(3) < 0.5).astype(np.int64)
    data = V.ImageDataObj(str(tmp_path), 'multi_label', {0: 'a', 1: 'b', 2: 'c'}, 8, V.get_transforms('TopDown', sz=32),
                          _decoded(24, 0, multi), _decoded(12, 1, multi), seed=3)
    torch.manual_seed(0)
    learner = V.ImageLearner(str(tmp_path), data, V.ImageClassificationNet(data, V.models.resnet18()))
    assert isinstance(learner.loss_func, HipBCEWithLogitsLoss)
    learner.freeze(); learner.bn_freeze()
    learner.fit(1e-3, 1, metrics=[fbeta_loss(2, 0.2)])
    assert len(learner.loss_sched) == 3 and np.isfinite(learner.loss_sched).all()
    learner.unfreeze(); learner.bn_unfreeze(); learner.use_graphs()
    learner.fit(1e-3, 2, metrics=[fbeta_loss(2, 0.2)])
    assert len(learner.loss_sched) == 6 and np.isfinite(learner.loss_sched).all()
    assert len(learner._graphs) == 1 and next(iter(learner._graphs.values())).graph is not None
    arena, val_arena = data.train_dl.arena.data_ptr(), data.val_dl.arena.data_ptr()
    learner.data_resize(64, bs=4)
    assert learner._graphs == {} and data.sz == (64, 64) and data.bs == 4
    assert data.train_dl.arena.data_ptr() == arena and data.val_dl.arena.data_ptr() == val_arena
    assert len(data.train_dl) == 6 and tuple(next(iter(data.val_dl))[0].shape) == (4, 3, 64, 64)
    learner.fit(1e-3, 1, metrics=[fbeta_loss(2, 0.2)])
    assert len(learner.loss_sched) == 6 and np.isfinite(learner.loss_sched).all()
    assert [k[0][0][0] for k in learner._graphs] == [(4, 3, 64, 64)]           # the step was captured again, at the new size
    res = learner.evaluate('val', metrics=[fbeta_loss(2, th) for th in THRESHOLDS])
    assert np.isfinite(res[0]) and 0 <= res[1] <= 1 and len(res[2]) == 5 and ((0 <= res[2]) & (res[2] <= 1)).all()

    probs, labels = learner.TTA('val')
    tfms, weights = learner.tta_transforms(0.4)
    views = [data.val_dl.with_transform(t, bs=data.bs, seed=data.val_dl.seed + k) for k, t in enumerate(tfms)]
    assert all(v.arena.data_ptr() == val_arena for v in views)
    want = V.combine_preds([learner.predict(v)[0] for v in views], 'multi_label', weights)
    assert probs.shape == (12, 3) and ((probs >= 0) & (probs <= 1)).all() and set(np.unique(labels)) <= {0, 1}
    assert np.abs(probs - want[0]).max() <= 1e-6 and np.array_equal(labels, want[1]) and np.array_equal(labels, probs.round().astype(int))
    assert np.abs(probs - learner.predict('val')[0]).max() > 1e-6             # the augmented views did contribute


@pytest.mark.gpu
def test_single_label_tta_and_confusion_matrix(tmp_path, quiet):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    single = lambda rs, i: i % 3
    data = V.ImageDataObj(str(tmp_path), 'single_label', {0: 'a', 1: 'b', 2: 'c'}, 8, V.get_transforms('SideOn', sz=32),
                          _decoded(8, 0, single), _decoded(12, 1, single), _decoded(5, 2, lambda rs, i: 0), test_name='test', seed=3)
    torch.manual_seed(0)
    learner = V.ImageLearner(str(tmp_path), data, V.ImageClassificationNet(data, V.models.resnet18()))
    probs, labels = learner.TTA('val')
    assert probs.shape == (12, 3) and np.allclose(probs.sum(1), 1, atol=1e-5) and np.array_equal(labels, probs.argmax(axis=1))
    assert learner.TTA('test', beta=0.5)[0].shape == (5, 3)
    learner.confusion_matrix(pred_labels=labels)
    assert len(plt.gcf().axes) >= 1
    plt.close('all')
    learner.confusion_matrix()
    plt.close('all')
