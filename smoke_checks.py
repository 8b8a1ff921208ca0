"""TEST INFRASTRUCTURE (lives next to __graft_entry__.py, outside the product package).  Small GPU-vs-oracle checks used by
__graft_entry__.smoke(): one tiny forward+backward of every hot-path head on the HIP kernels (through the C ABI), compared with
the CPU oracle (imported here as the CHECKER only)."""
import numpy as np
import torch
import torch.nn as nn


def _close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    if not bool((err <= atol + rtol * b.abs()).all()):
        raise AssertionError(f'smoke: {what} mismatch, max abs err {err.max().item():.3e}')


def check_collab(device):
    from oracle import reference_math as RM
    from neuralnetworklibrary_amd import ops
    g = torch.Generator().manual_seed(0)
    n, nu, ni, D = 64, 943, 1682, 30
    x = torch.stack([torch.randint(0, nu, (n,), generator=g), torch.randint(0, ni, (n,), generator=g)], 1)
    ps = [torch.randn(nu, D, generator=g) * .3, torch.randn(ni, D, generator=g) * .3,
          torch.randn(nu, 1, generator=g), torch.randn(ni, 1, generator=g)]
    dy = torch.randn(n, generator=g)
    cpu = [p.clone().requires_grad_(True) for p in ps]
    ref = RM.embdotbias(x, *cpu, [0.8, 5.2]); ref.backward(dy)
    gpu = [p.clone().to(device).requires_grad_(True) for p in ps]
    out = ops.embdotbias(x.to(device), *gpu, [0.8, 5.2]); out.backward(dy.to(device))
    _close(out, ref, 1e-5, 1e-5, 'embdotbias fwd')
    for a, b in zip(gpu, cpu):
        _close(a.grad, b.grad, 1e-3, 1e-5, 'embdotbias grad')


def check_resnet_block(device):
    """conv3x3 -> BN -> ReLU -> conv3x3 -> BN -> +downsample(x) -> ReLU, stride 2 (conv fwd/dgrad/wgrad + fused BN)."""
    from oracle import reference_nets as RN
    from oracle import synth
    from neuralnetworklibrary_amd.Applications.VisionModels import retinanet as PN
    ds_p = PN._Downsample(PN.HipConv2d(16, 32, kernel_size=1, stride=2, bias=False), nn.BatchNorm2d(32))
    ds_o = nn.Sequential(nn.Conv2d(16, 32, 1, stride=2, bias=False), nn.BatchNorm2d(32))
    prod, orac = PN.BasicBlock(16, 32, 2, ds_p), RN.BasicBlock(16, 32, 2, ds_o)
    synth.fill_module_(prod, 1); synth.fill_module_(orac, 1)
    x = synth.synth_input((4, 16, 20, 20), 5)
    xo = x.clone().requires_grad_(True)
    yo = orac.train()(xo); dy = synth.synth_input(tuple(yo.shape), 6); yo.backward(dy)
    xp = x.to(device).requires_grad_(True)
    yp = prod.to(device).train()(xp); yp.backward(dy.to(device))
    _close(yp, yo, 1e-4, 1e-5, 'block y'); _close(xp.grad, xo.grad, 1e-3, 1e-5, 'block dx')
    for (n, p), (_, q) in zip(prod.named_parameters(), orac.named_parameters()):
        _close(p.grad, q.grad, 1e-3, 1e-4 * q.grad.abs().max().item(), 'block grad ' + n)


def check_tabular(device):
    from oracle import reference_nets as RN
    from oracle import synth
    from neuralnetworklibrary_amd.Applications.StructuredData import StructuredDataNet
    cards, n_cont, bs = [20, 5, 4, 13], 3, 32
    dims = [RN.embedding_dim(c) for c in cards]
    prod = StructuredDataNet('cont', 4, n_cont, [{i: i for i in range(c)} for c in cards], [32, 16, 1], output_range=[5, 12])
    orac = RN.StructuredDataNet('cont', list(zip(cards, dims)), n_cont, [32, 16, 1], output_range=[5, 12])
    synth.fill_module_(prod, 2); synth.fill_module_(orac, 2)
    rs = np.random.RandomState(0)
    xcat = torch.from_numpy(np.stack([rs.randint(0, c, size=bs) for c in cards], 1).astype(np.int64))
    xcont = torch.from_numpy(rs.standard_normal((bs, n_cont)).astype(np.float32))
    y = torch.from_numpy((5 + 7 * rs.rand(bs)).astype(np.float32))
    lo = nn.MSELoss()(orac.train()(xcat, xcont), y); lo.backward()
    lp = nn.MSELoss()(prod.to(device).train()(xcat.to(device), xcont.to(device)), y.to(device)); lp.backward()
    _close(lp, lo, 1e-4, 1e-6, 'tabular loss')
    for (n, p), (_, q) in zip(prod.named_parameters(), orac.named_parameters()):
        _close(p.grad, q.grad, 1e-3, 1e-5 * max(q.grad.abs().max().item(), 1e-3), 'tabular grad ' + n)


def check_retina_loss(device):
    from oracle import reference_math as RM
    from neuralnetworklibrary_amd import ops
    rs = np.random.RandomState(2)
    anchors = RM.anchors_for(64, 64)
    A, K, bs = len(anchors), 5, 2
    boxes = -np.ones((bs, 3, 4), np.float32); cats = -np.ones((bs, 3), np.int64)
    boxes[1, :2] = [[4, 6, 40, 44], [20, 10, 60, 34]]; cats[1, :2] = [2, 0]
    reg = torch.from_numpy(rs.standard_normal((bs, A, 4)).astype(np.float32) * .3)
    clas = torch.from_numpy(rs.uniform(0.01, 0.5, (bs, A, K)).astype(np.float32))
    rc, cc = reg.clone().requires_grad_(True), clas.clone().requires_grad_(True)
    tot, r, c = RM.ssd_loss(anchors, rc, cc, torch.from_numpy(boxes), torch.from_numpy(cats)); tot.backward()
    rg, cg = reg.to(device).requires_grad_(True), clas.to(device).requires_grad_(True)
    out = ops.retina_loss(anchors.to(device), rg, cg, torch.from_numpy(boxes).to(device), torch.from_numpy(cats).to(device))
    out[0].backward()
    _close(out, torch.stack([tot, r, c]), 1e-4, 1e-6, 'retina loss')
    _close(rg.grad, rc.grad, 1e-4, 1e-9, 'retina dreg'); _close(cg.grad, cc.grad, 1e-4, 1e-8, 'retina dclas')


def check_lstm_lm(device):
    from oracle import reference_text as RT
    from oracle import synth
    from neuralnetworklibrary_amd.Applications.Text import LanguageModelNet, RegSeqCrossEntropyLoss, _Vocab
    V, bs, seq = 40, 4, 6
    stoi = {('t%d' % i): i for i in range(V)}
    stoi['_pad_'] = 1
    del stoi['t1']
    d = _Vocab(stoi, bs)
    prod = LanguageModelNet(d, enc_drops=[0., 0., 0., 0.], dec_drop=0., emb_dim=16, hidden_size=24, num_layers=3)
    orac = RT.LanguageModelNet(V, 1, bs, E=16, Hh=24, L=3)
    synth.fill_module_(prod, 3); synth.fill_module_(orac, 3)
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.randint(0, V, (bs, seq)).astype(np.int64)); y = torch.from_numpy(rs.randint(0, V, (bs, seq)).astype(np.int64))
    lo, _ = RT.reg_seq_cross_entropy(orac.train()(x), y); lo.backward()
    lp = RegSeqCrossEntropyLoss()(prod.to(device).train()(x.to(device)), y.to(device)); lp.backward()
    _close(lp, lo, 1e-4, 1e-6, 'LM loss')
    for (n, p), (_, q) in zip(prod.named_parameters(), orac.named_parameters()):
        _close(p.grad, q.grad, 1e-3, 1e-5 * max(q.grad.abs().max().item(), 1e-3), 'LM grad ' + n)


def check_tabular_assoc(device):
    """get_association of the three families on a 64-row frame with missing values (K13: contingency counts, per-category moments,
    two-pass correlations), against numpy written out here."""
    import pandas as pd
    from neuralnetworklibrary_amd.Applications import StructuredData as SD
    rs = np.random.RandomState(3)
    n = 64
    a, b = rs.randint(0, 4, n).astype('float64'), rs.randint(0, 3, n).astype('float64')
    x = rs.standard_normal(n) + a
    y = x * x + rs.standard_normal(n)
    a[::9], x[1::7] = np.nan, np.nan
    df = pd.DataFrame({'a': a, 'b': b, 'x': x, 'y': y})
    ok = ~np.isnan(a)
    t = np.bincount((a[ok] * 3 + b[ok]).astype(int), minlength=12).reshape(4, 3) / ok.sum()
    h = lambda p: -(np.log(p[p > 0]) * p[p > 0]).sum()      # noqa: E731  (no empty cell here: no clamp term)
    assert (t > 0).all()
    i_ab = h(t.sum(1)) + h(t.sum(0)) - h(t.ravel())
    want_mi = 0.5 * (i_ab / h(t.sum(1)) + i_ab / h(t.sum(0)))
    ok = ~np.isnan(a) & ~np.isnan(x)
    av, xv = a[ok], x[ok]
    between = sum((av == k).sum() * (xv[av == k].mean() - xv.mean()) ** 2 for k in range(4)) / ok.sum()
    want_ratio = np.sqrt(between / xv.var(ddof=1))
    ok = ~np.isnan(x)
    dx, dy = x[ok] - x[ok].mean(), y[ok] - y[ok].mean()
    ax, ay = np.abs(dx) - np.abs(dx).mean(), np.abs(dy) - np.abs(dy).mean()
    corr = lambda u, v: abs(u @ v) / np.sqrt((u @ u) * (v @ v))      # noqa: E731
    want_corr = max(corr(dx, dy), corr(dx, ay), corr(ax, dy), corr(ax, ay))
    for Type, X, Y, want in (('mutual_info_symmetric', 'a', 'b', want_mi), ('correlation_ratio', 'a', 'x', want_ratio),
                             ('abs_max_correlation', 'x', 'y', want_corr)):
        got = SD.get_association(df, X, Y, Type)
        if not abs(got - want) <= 1e-12:
            raise AssertionError(f'smoke: {Type} mismatch, got {got!r}, want {want!r}')


def check_det_eval(device):
    """two images, two detections and two ground truths of one category through the COCO protocol and the mAP (K14): the perfect
    detection scores above the one that overlaps 7 / 8, so AP is 1 up to t = 0.85 and 1 / 2 above."""
    from neuralnetworklibrary_amd import ops
    f = lambda *v: np.array(v, dtype=np.float32)      # noqa: E731
    coco = {'images': [{'id': 2}, {'id': 1}], 'categories': [{'id': 6}],
            'annotations': [{'id': 1, 'image_id': 2, 'category_id': 6, 'bbox': [10., 10., 50., 40.], 'area': 2000., 'iscrowd': 0},
                            {'id': 2, 'image_id': 1, 'category_id': 6, 'bbox': [0., 0., 20., 20.], 'area': 400., 'iscrowd': 0}]}
    preds = [[[f(10, 10, 60, 45)], [0], [np.float32(0.5)]], [[f(0, 0, 20, 20)], [0], [np.float32(0.75)]]]
    packed = ops.det_eval_pack(preds, coco=coco, image_ids=[2, 1], cat2dscat={0: 6})
    thr = np.linspace(.5, .95, 10)
    rec = np.linspace(0, 1, 101)
    precision, recall, _ = ops.det_eval_coco(packed, thr, rec, [1, 10, 100], [[0, 1e10]], device=device)
    half = np.where(rec <= 0.5, 1 / (1 + np.spacing(1)), 0.0).mean()      # one hit, then one miss: precision 1 / (1 + eps) up to recall 1 / 2
    want = np.where(thr <= 0.875, 1.0, half)
    if not np.array_equal(precision[:, :, 0, 0, 2].mean(axis=1), want) or not np.array_equal(recall[:, 0, 0, 2], np.where(thr <= 0.875, 1.0, 0.5)):
        raise AssertionError(f'smoke: det_eval_coco mismatch, got {precision[:, :, 0, 0, 2].mean(axis=1)!r}, want {want!r}')
    targets = [[(np.array([10., 10., 60., 50.]), 0)], [(np.array([0., 0., 20., 20.]), 0)]]
    vals = ops.det_map(ops.det_eval_pack(preds, targets=targets, n_categories=1), [0.5, 0.9], device=device)
    if vals.tolist() != [[1.0], [0.5]]:
        raise AssertionError(f'smoke: det_map mismatch, got {vals!r}')


CHECKS = [check_collab, check_resnet_block, check_tabular, check_retina_loss, check_lstm_lm, check_tabular_assoc, check_det_eval]


def run_all(device='cuda:0'):
    from neuralnetworklibrary_amd import ops
    for c in CHECKS:
        c(device)
        print('  smoke check passed:', c.__name__)
    ops.raise_if_index_error()
    torch.cuda.synchronize()
