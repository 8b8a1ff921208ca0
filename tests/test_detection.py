"""Detection loss (K6) and anchors: oracle pinned to the reference golden G8 on CPU; fused HIP kernel vs golden and
vs the oracle at the BASELINE size (512x512 -> 49 104 anchors, K=20, bs=16) on GPU."""
import numpy as np
import pytest
import torch

from conftest import T, assert_close, load_golden
from oracle import reference_math as RM

DEV = 'cuda'


def check_anchors(make, g):
    for sz in [64, 512]:
        a = make(sz).detach().cpu().numpy()
        assert list(a.shape) == list(g['anchors%d.shape' % sz])
        np.testing.assert_array_equal(a[:40], g['anchors%d.head' % sz])          # bit-exact
        np.testing.assert_array_equal(a[-40:], g['anchors%d.tail' % sz])
        np.testing.assert_allclose(a.astype(np.float64).sum(0), g['anchors%d.sum' % sz], rtol=0, atol=0)
        np.testing.assert_allclose(np.abs(a.astype(np.float64)).sum(0), g['anchors%d.abs_sum' % sz], rtol=0, atol=0)
    assert g['anchors512.shape'][0] == 49104


def state_from_golden(g, i, N):
    st = np.full(N, -2, dtype=np.int64)
    st[g['img%d.neg' % i]] = -1
    pos = g['img%d.pos' % i]
    st[pos] = g['img%d.matches' % i][pos]
    return st


def test_g8_anchors_oracle():
    check_anchors(lambda sz: RM.anchors_for(sz, sz), load_golden('g8_detection'))


def test_g8_loss_oracle():
    g = load_golden('g8_detection')
    anchors = RM.anchors_for(64, 64)
    reg, clas = T(g['reg']).requires_grad_(True), T(g['clas']).requires_grad_(True)
    B, C = T(g['boxes']), T(g['cats'])
    for i in range(len(B)):
        st = RM.match_anchors_objects(B[i][C[i] >= 0], anchors)
        np.testing.assert_array_equal(st.numpy(), state_from_golden(g, i, len(anchors)))
    total, r, c = RM.ssd_loss(anchors, reg, clas, B, C, 0.5, 0.25, 2.0)
    assert_close(total, g['loss'], 1e-6, 1e-7, 'loss')
    assert_close(r, g['reg_loss'], 1e-6, 1e-7, 'reg')
    assert_close(c, g['clas_loss'], 1e-6, 1e-7, 'clas')
    total.backward()
    assert_close(reg.grad, g['dreg'], 1e-5, 1e-9, 'dreg')
    assert_close(clas.grad, g['dclas'], 1e-5, 1e-9, 'dclas')


@pytest.mark.gpu
def test_g8_anchors_hip_side():
    from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import AnchorGenerator
    gen = AnchorGenerator()
    check_anchors(lambda sz: gen(torch.zeros(1, 3, sz, sz, device=DEV)), load_golden('g8_detection'))
    assert gen(torch.zeros(1, 3, 64, 64, device=DEV)) is gen(torch.zeros(2, 3, 64, 64, device=DEV))     # cached on device


@pytest.mark.gpu
def test_g8_loss_hip():
    from neuralnetworklibrary_amd.Applications.Vision import SSD_loss, ssd1
    g = load_golden('g8_detection')
    anchors = RM.anchors_for(64, 64).to(DEV)
    reg, clas = T(g['reg'], DEV).requires_grad_(True), T(g['clas'], DEV).requires_grad_(True)
    B, C = T(g['boxes'], DEV), T(g['cats'], DEV)
    lf = SSD_loss(0.5, 0.25, 2.0)
    loss = lf([anchors, reg, clas], [B, C])
    assert_close(loss, g['loss'], 1e-5, 1e-7, 'loss')
    assert_close(lf.reg_loss, g['reg_loss'], 1e-5, 1e-7, 'reg')
    assert_close(lf.clas_loss, g['clas_loss'], 1e-5, 1e-7, 'clas')
    loss.backward()
    assert_close(reg.grad, g['dreg'], 1e-4, 1e-9, 'dreg')
    assert_close(clas.grad, g['dclas'], 1e-4, 1e-8, 'dclas')
    for i in range(len(B)):                                  # per-image API (ssd1) incl. the image without objects
        keep = C[i] >= 0
        r, c = ssd1(anchors, B[i][keep], C[i][keep], reg[i].detach(), clas[i].detach())
        assert_close(r, g['img%d.reg_loss' % i], 1e-5, 1e-7, 'img reg')
        assert_close(c, g['img%d.clas_loss' % i], 1e-5, 1e-7, 'img clas')


@pytest.mark.gpu
def test_matching_state_bit_exact():
    """The kernel's pos / neg / ignore decision per anchor must equal the reference's: it thresholds the same IEEE ops."""
    from neuralnetworklibrary_amd import ops
    g = load_golden('g8_detection')
    anchors = RM.anchors_for(64, 64).to(DEV)
    reg, clas, B, C = T(g['reg'], DEV), T(g['clas'], DEV), T(g['boxes'], DEV), T(g['cats'], DEV)
    f = ops._RetinaLoss
    ctx = type('C', (), {'save_for_backward': lambda self, *a: setattr(self, 'saved', a)})()
    f.forward(ctx, anchors, reg, clas, B, C, 0.5, 0.25, 2.0)
    state = ctx.saved[5].cpu().numpy()
    for i in range(len(B)):
        np.testing.assert_array_equal(state[i], state_from_golden(g, i, anchors.shape[0]))


@pytest.mark.gpu
def test_full_size_vs_oracle():
    """BASELINE config 5 loss shapes: 512x512 -> 49 104 anchors, K=20, bs=16, 1..8 boxes per image."""
    from neuralnetworklibrary_amd import ops
    rs = np.random.RandomState(5)
    bs, K, M = 16, 20, 8
    anchors = RM.anchors_for(512, 512)
    A = len(anchors)
    boxes = -np.ones((bs, M, 4), np.float32); cats = -np.ones((bs, M), np.int64)
    for i in range(bs):
        m = rs.randint(1, M + 1)
        xy = rs.uniform(0, 300, (m, 2)); wh = rs.uniform(30, 210, (m, 2))
        boxes[i, :m] = np.concatenate([xy, xy + wh], 1); cats[i, :m] = rs.randint(0, K, m)
    reg = torch.from_numpy(rs.standard_normal((bs, A, 4)).astype(np.float32) * 0.3)
    clas = torch.from_numpy(rs.uniform(0.001, 0.2, (bs, A, K)).astype(np.float32))
    rc, cc = reg.clone().requires_grad_(True), clas.clone().requires_grad_(True)
    total, r, c = RM.ssd_loss(anchors, rc, cc, torch.from_numpy(boxes), torch.from_numpy(cats))
    total.backward()
    rg, cg = reg.to(DEV).requires_grad_(True), clas.to(DEV).requires_grad_(True)
    out = ops.retina_loss(anchors.to(DEV), rg, cg, torch.from_numpy(boxes).to(DEV), torch.from_numpy(cats).to(DEV))
    out[0].backward()
    assert_close(out, torch.stack([total, r, c]), 1e-4, 1e-6, 'losses')
    assert_close(rg.grad, rc.grad, 1e-4, 1e-10, 'dreg')
    assert_close(cg.grad, cc.grad, 1e-4, 1e-9, 'dclas')


def assert_within_reference_gap(got, g, key, msg, slack=3.0, floor=1e-3, normwise=False, host32=None):
    """|got - f64| <= slack * gap + floor * |f64| elementwise, gap = the reference's own |fp32 - fp64| (never below its 95th
    percentile over the tensor: a single fp32 run is one noisy sample of its error).
    normwise=True (gradient tensors): ||got - f64|| <= slack ||f32 - f64|| + floor ||f64|| over the whole tensor.  A gradient is
    a discontinuous function of the weights (ReLU gates: an activation within rounding of zero gets the opposite gate in two
    correct fp32 evaluations and moves every weight-gradient element it feeds), so single elements of two correct fp32 results
    legitimately differ by more than 1e-3 of their own magnitude; the tensor as a whole may not.
    host32: the same quantity from the CPU oracle in fp32 ON THIS HOST.  At G12's size (C5 is 2x2 pixels, P6 / P7 one pixel) one
    gate decides ~1e-3 of every upstream gradient, and torch's own fp32 CPU run is not reproducible across hosts at that level:
    measured on the GPU box, torch-CPU fp32 sits 5.4e-3 from the golden fp64 on fpn.P5_1.weight where the golden fp32 (made in
    the build container: other ISA, other mkldnn blocking) sits 2.8e-6 — and the HIP result equals the box's torch-CPU fp32 to
    2e-6.  The gap is therefore the larger of the two fp32 separations: "as far from fp64 as torch fp32 on this machine"."""
    r32, r64 = g[key + '.f32'], g[key + '.f64']
    got = got.detach().cpu().double().numpy().reshape(r64.shape)
    if normwise:
        err, gapn, ref = np.linalg.norm(got - r64), np.linalg.norm(r32 - r64), np.linalg.norm(r64)
        if host32 is not None:
            gapn = max(gapn, np.linalg.norm(host32.detach().cpu().double().numpy().reshape(r64.shape) - r64))
        assert err <= slack * gapn + floor * ref, '%s: ||got-f64|| %.3e > %g x ||f32-f64|| %.3e + %g x ||f64|| %.3e' % (
            msg, err, slack, gapn, floor, ref)
        return
    gap = np.abs(r32 - r64)
    tol = slack * np.maximum(gap, np.quantile(gap, 0.95)) + floor * np.abs(r64) + 1e-12
    err = np.abs(got - r64)
    assert (err <= tol).all(), '%s: %d elements outside the reference fp32/fp64 gap, worst err/tol %.2f' % (
        msg, (err > tol).sum(), (err / tol).max())


def test_g12_oracle_objectdetectionnet_is_pinned_to_the_reference():
    """The oracle's restated ObjectDetectionNet (oracle/reference_nets.py: ResNet-50 body, PyramidFeatures, the two head towers)
    + restated SSD loss reproduce the reference's own fp32 run (G12) — same parameter enumeration, activations, loss and
    gradient norms, BatchNorm in training mode then in eval mode as the generator ran it."""
    from oracle import reference_math as RM, reference_nets as RN, synth
    g = load_golden('g12_objectdetectionnet')
    net = RN.ObjectDetectionNet(int(g['K']))
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in g['param_names']]
    synth.fill_detection_net_(net)
    x = synth.synth_input((int(g['N']), 3, int(g['S']), int(g['S'])), 12)
    B, Cc = torch.from_numpy(g['boxes']), torch.from_numpy(g['cats'])
    for mode in ['train', 'eval']:
        net.train() if mode == 'train' else net.eval()
        for p in net.parameters():
            p.grad = None
        anchors, reg, clas = net(x)
        loss = RM.ssd_loss(anchors, reg, clas, B, Cc, 0.5, 0.25, 2.0)[0]
        loss.backward()
        assert_close(reg, g[mode + '.reg.f32'], 1e-5, 1e-6, mode + ' reg')
        assert_close(clas, g[mode + '.clas.f32'], 1e-5, 1e-7, mode + ' clas')
        assert_close(loss, g[mode + '.loss.f32'].reshape(()), 1e-5, 1e-7, mode + ' loss')
        norms = np.array([0.0 if p.grad is None else p.grad.norm().item() for _, p in net.named_parameters()])
        assert_close(norms, g[mode + '.grad_norms.f32'], 1e-4, 1e-6, mode + ' grad norms')


@pytest.mark.gpu
def test_g12_objectdetectionnet_hip_vs_reference():
    """The assembled RetinaNet (ResNet-50 Bottleneck body + FPN + heads) + SSD loss against the reference's own fp32 / fp64 runs
    (golden G12): activations, loss and per-parameter gradient norms with BatchNorm in training mode (fp32-vs-fp64 gap
    criterion) and in eval mode (plus gradient slices)."""
    from neuralnetworklibrary_amd.Applications import Vision as V
    from oracle import synth
    g = load_golden('g12_objectdetectionnet')

    N, S, K = int(g['N']), int(g['S']), int(g['K'])
    torch.manual_seed(0)
    net = V.ObjectDetectionNet(K)
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in g['param_names']]
    synth.fill_detection_net_(net)             # the generator's well-conditioned seeded weights: every activation O(1)
    net = net.to(DEV)
    x = synth.synth_input((N, 3, S, S), 12).to(DEV)
    B, Cc = T(g['boxes'], DEV), T(g['cats'], DEV)
    sd = dict(net.named_parameters())
    from oracle import reference_math as RM, reference_nets as RN
    onet = synth.fill_detection_net_(RN.ObjectDetectionNet(K))          # torch-CPU fp32 on this host: the second adjudicator
    osd = dict(onet.named_parameters())
    slice_names = [str(s) for s in g['slice_names'] if 'eval.grad.%s.f32' % s in g]
    host_draws = eps_perturbed_eval_slices(K, x.cpu(), B.cpu(), Cc.cpu(), slice_names)
    for mode in ['train', 'eval']:
        net.train() if mode == 'train' else net.eval()
        onet.train() if mode == 'train' else onet.eval()
        for p in list(net.parameters()) + list(onet.parameters()):
            p.grad = None
        oa, oreg, oclas = onet(x.cpu())
        RM.ssd_loss(oa, oreg, oclas, B.cpu(), Cc.cpu(), 0.5, 0.25, 2.0)[0].backward()
        anchors, reg, clas = net(x)
        assert tuple(anchors.shape) == tuple(int(v) for v in g['anchors.shape'])
        lf = V.SSD_loss(0.5, 0.25, 2.0)
        loss = lf([anchors, reg, clas], [B, Cc])
        loss.backward()
        # |hip - f64| <= 3 x the reference's own fp32-vs-fp64 gap + 1e-3 |f64| (north_star's relative tolerance), no absolute slack
        slack = 3.0
        assert_within_reference_gap(reg, g, mode + '.reg', mode + ' reg', slack=slack)
        assert_within_reference_gap(clas, g, mode + '.clas', mode + ' clas', slack=slack)
        assert_within_reference_gap(loss.reshape(1), g, mode + '.loss', mode + ' loss', slack=slack)
        norms = torch.tensor([0.0 if p.grad is None else p.grad.norm().item() for _, p in net.named_parameters()], dtype=torch.float64)
        assert_within_reference_gap(norms, g, mode + '.grad_norms', mode + ' grad norms', slack=slack)
        if mode == 'eval':
            worst = []
            for n in slice_names:
                hosts32 = [osd[n].grad.reshape(-1)[:1024]] + [d[n] for d in host_draws]
                worst.append((slice_gap_ratio(sd[n].grad.reshape(-1)[:1024], g, 'eval.grad.' + n, slack, GRAD_SLICE_FLOOR, hosts32), n))
            worst.sort(reverse=True)
            print('G12 eval gradient slices, err / (%g x gap + %g x norm), worst first:' % (slack, GRAD_SLICE_FLOOR),
                  ', '.join('%s %.2f' % (n, r) for r, n in worst[:5]))
            assert worst[0][0] <= 1.0, 'eval grad %s: %.2f x the allowed distance from fp64 (worst five: %s)' % (
                worst[0][1], worst[0][0], worst[:5])


FLOORED_TENSORS = ('regressor.',)          # see the end of the test below

# Gradient SLICES (1024 elements of one weight gradient, eval mode) are the noisiest quantity this file checks: one ReLU gate that
# two correct fp32 evaluations set differently moves a slice by ~1e-3 of its norm (docstring of assert_within_reference_gap), and
# which gates sit within rounding of zero changes with every legitimate change of summation order.  The test prints the worst
# five ratios err / (3 x gap + floor x norm).  Measured on the GPU box at G12's size (64 x 64 input: every 3x3 convolution is
# tiny, so the dispatcher keeps them on the direct kernel): worst 0.37 at a floor of 2e-3.  With the Winograd kernel FORCED onto
# these tiny maps (NNL_CONV_WINO=2) the worst slice is fpn.P5_1.weight at 1.37 (2e-3 floor) although the two kernels agree to
# 1e-6 on every single convolution of that size (tools/wino_debug.py) — gate flips on a 2x2 map, not arithmetic error; the
# production sizes (G13b, G15: 20- / 10-step loss curves) run the Winograd kernel and hold their 1e-3.
# The host's torch-CPU fp32 run is ONE draw of those gate flips, and which draw it is depends on the host: on fpn.P5_1.weight the
# unperturbed run flips the decisive gate at one OpenMP thread (5.5e-3 from fp64) and not at 2 - 16 threads (6e-7), so the check
# passed or failed (4.1) with the thread count of the machine.  The adjudicator is therefore the envelope of that run and four
# torch-CPU fp32 runs from weights moved by <= 1 ulp (the yardstick of the full-size test below and of G13), which draws the flip
# at any thread count.
GRAD_SLICE_FLOOR = 1e-3
EPS_DRAW_SEEDS = (100, 101, 102, 103)


def eps_perturbed_eval_slices(K, x, B, Cc, names, seeds=EPS_DRAW_SEEDS):
    """torch-CPU fp32 oracle from the G12 weights moved by <= 1 ulp (one draw per seed), run as the generator ran it (training
    mode, then eval mode): per draw {name: the first 1024 elements of the eval-mode weight gradient}"""
    from oracle import reference_math as RM, reference_nets as RN, synth
    draws = []
    for seed in seeds:
        net = synth.fill_detection_net_(RN.ObjectDetectionNet(K))
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(1.0 + 2.0 ** -23 * (torch.randint(0, 3, p.shape, generator=gen).float() - 1.0))
        for mode in ['train', 'eval']:
            net.train() if mode == 'train' else net.eval()
            for p in net.parameters():
                p.grad = None
            a, r, c = net(x)
            RM.ssd_loss(a, r, c, B, Cc, 0.5, 0.25, 2.0)[0].backward()
        sd = dict(net.named_parameters())
        draws.append({n: sd[n].grad.reshape(-1)[:1024].detach().clone() for n in names})
    return draws


def slice_gap_ratio(got, g, key, slack, floor, hosts32):
    "||got - f64|| / (slack x max(||f32 - f64||, max over hosts32 ||host32 - f64||) + floor x ||f64||) for one gradient slice"
    r32, r64 = g[key + '.f32'], g[key + '.f64']
    got = got.detach().cpu().double().numpy().reshape(r64.shape)
    gapn = max([np.linalg.norm(r32 - r64)] + [np.linalg.norm(h.detach().cpu().double().numpy().reshape(r64.shape) - r64) for h in hosts32])
    return float(np.linalg.norm(got - r64) / (slack * gapn + floor * np.linalg.norm(r64)))


@pytest.mark.gpu
def test_objectdetectionnet_full_baseline_size_vs_oracle_fp64():
    """BASELINE configs[4] assembled at its own image size — ObjectDetectionNet(20): ResNet-50 Bottleneck body + FPN + shared
    heads on five levels, 512 x 512 (49 104 anchors), 2 images, BatchNorm in training mode, SSD_loss(0.5, 0.25, 2) — one forward
    + backward of the HIP path against the CPU oracle in fp32 AND fp64 on the same (well-conditioned, seeded) weights.
    Activations elementwise and every parameter gradient in norm: |hip - f64| <= 3 |cpu32 - f64| + 1e-3 |f64|."""
    from neuralnetworklibrary_amd.Applications import Vision as V
    from oracle import reference_math as RM, reference_nets as RN, synth
    K, N, S = 20, 2, 512
    x = synth.synth_input((N, 3, S, S), 77)
    boxes = -np.ones((N, 4, 4), np.float32); cats = -np.ones((N, 4), np.int64)
    boxes[0, :3] = [[30, 40, 200, 260], [250, 100, 420, 300], [100, 300, 180, 380]]; cats[0, :3] = [3, 17, 0]
    boxes[1, :2] = [[60, 60, 460, 440], [10, 400, 90, 500]]; cats[1, :2] = [9, 19]
    B, Cc = torch.from_numpy(boxes), torch.from_numpy(cats)
    o32 = synth.fill_detection_net_(RN.ObjectDetectionNet(K), seed=3).train()
    o64 = synth.fill_detection_net_(RN.ObjectDetectionNet(K), seed=3).double().train()
    torch.manual_seed(0)
    net = synth.fill_detection_net_(V.ObjectDetectionNet(K), seed=3).to(DEV).train()
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in o32.named_parameters()]
    anchors, reg, clas = net(x.to(DEV))
    loss = V.SSD_loss(0.5, 0.25, 2.0)([anchors, reg, clas], [B.to(DEV), Cc.to(DEV)])
    loss.backward()
    a32, r32, c32 = o32(x)
    l32 = RM.ssd_loss(a32, r32, c32, B, Cc, 0.5, 0.25, 2.0)[0]
    l32.backward()
    a64, r64, c64 = o64(x.double())
    l64 = RM.ssd_loss(a64, r64, c64, B.double(), Cc, 0.5, 0.25, 2.0)[0]
    l64.backward()
    # Four more fp32 samples of the SAME problem: torch-CPU fp32 from weights moved by <= 1 ulp.  Why: behind a ReLU layer the
    # gradient of any fp32 evaluation carries a relative error floor of ~sqrt(P(gate flips)) ~ 1e-3 in norm, whatever the tensor
    # size (a pre-activation within rounding of zero — probability ~2e-7 per element — gets the opposite gate, and one flipped
    # gate among n moves the gradient by ~1/sqrt(n) of its norm); with box-regression gradients living on ~100 positive anchors a
    # single flip can show as 1e-2.  One fp32 run is ONE draw of those flips (measured here: torch-CPU fp32 drew none in the
    # regressor tower, 2e-6, where the HIP run drew one, 1e-2; in the ResNet-34 body both sit at 6e-3).  The envelope of several
    # draws is the fair estimate of what a correct fp32 evaluation may deviate by.
    samples = [[p.grad.double() for p in o32.parameters()]]
    for seed in range(4):
        op = synth.fill_detection_net_(RN.ObjectDetectionNet(K), seed=3).train()
        gen = torch.Generator().manual_seed(100 + seed)
        with torch.no_grad():
            for p in op.parameters():
                p.mul_(1.0 + 2.0 ** -23 * (torch.randint(0, 3, p.shape, generator=gen).float() - 1.0))
        ap, rp, cp_ = op(x)
        RM.ssd_loss(ap, rp, cp_, B, Cc, 0.5, 0.25, 2.0)[0].backward()
        samples.append([p.grad.double() for p in op.parameters()])
    assert anchors.shape[0] == 49104 and torch.equal(anchors.cpu(), a32)
    for name, hip, c, d in (('reg', reg, r32, r64), ('clas', clas, c32, c64), ('loss', loss, l32, l64)):
        hip, c, d = hip.detach().cpu().double(), c.detach().double(), d.detach()
        gap = (c - d).abs()
        tol = 3 * torch.clamp(gap, min=torch.quantile(gap.reshape(-1)[:4000000], 0.95).item() if gap.numel() > 1 else 0.0) + 1e-3 * d.abs()
        assert ((hip - d).abs() <= tol).all(), '%s: worst err/tol %.2f' % (name, ((hip - d).abs() / tol).max().item())
    rows = []
    for i, ((n, pp), (_, p64)) in enumerate(zip(net.named_parameters(), o64.named_parameters())):
        g64, gp = p64.grad, pp.grad.detach().cpu().double()
        rows.append((n, (gp - g64).norm().item(), max((smp[i] - g64).norm().item() for smp in samples), g64.norm().item()))
    # the run's own spread (q90 of the envelope over all tensors) is a floor ONLY for the tensors whose gradient
    # lives on the ~100 positive anchors of the batch — the box-regression tower (`regressor.*`: smooth-L1 is summed over positives
    # only, Vision.py:1532-1566) — where one gate flip shows as 1e-2 whatever the tensor's own five-sample envelope happened to
    # draw.  Every other tensor (backbone, FPN, classifier tower: gradients averaged over 49 104 anchors x 20 classes) must sit
    # within 3x its OWN envelope + 1e-3.
    q90 = float(np.quantile([e_cpu / max(ref, 1e-300) for _, _, e_cpu, ref in rows], 0.9))
    bad = []
    for n, e_hip, e_cpu, ref in rows:
        floor = q90 * ref if n.startswith(FLOORED_TENSORS) else 0.0
        if not e_hip <= 3 * max(e_cpu, floor) + 1e-3 * ref:
            bad.append('%s: |hip-f64| %.3e vs max |cpu32-f64| %.3e (|f64| %.3e, rel %.2e / %.2e)' % (n, e_hip, e_cpu, ref, e_hip / max(ref, 1e-300), e_cpu / max(ref, 1e-300)))
    print('worst relative gradient error vs fp64: hip %.2e, cpu32 envelope %.2e (q90 %.2e)' % (
        max(e / max(r, 1e-300) for _, e, _, r in rows), max(e / max(r, 1e-300) for _, _, e, r in rows), q90))
    assert not bad, '%d tensors outside 3x their own fp32 envelope + 1e-3:\n%s' % (len(bad), '\n'.join(bad))


def _g15_net_and_loss(g):
    from neuralnetworklibrary_amd.Applications import Vision as V
    from oracle import synth
    torch.manual_seed(0)
    net = synth.fill_detection_net_(V.ObjectDetectionNet(int(g['K'])), seed=int(g['init_seed'])).to(DEV).train()
    assert [n for n, _ in net.named_parameters()] == [str(s) for s in g['param_names']]
    return net, V.SSD_loss(0.5, 0.25, 2.0)


def _g15_batch(g, tag):
    from oracle import synth
    N, S, K, M = int(g['N']), int(g['S']), int(g['K']), int(g['M'])
    boxes, cats = synth.detection_targets(N, M, S, K, tag)
    return synth.synth_input((N, 3, S, S), tag).to(DEV), [torch.from_numpy(boxes).to(DEV), torch.from_numpy(cats).to(DEV)]


@pytest.mark.gpu
def test_g15_objectdetectionnet_assembled_at_baseline_batch_16_vs_reference():
    """VERDICT r2 missing #4 / next #1(b): the ASSEMBLED ObjectDetectionNet(20) + SSD_loss at BASELINE configs[4]'s own size —
    512 x 512, bs 16 (the batch the bench times: planner choices depend on N), 49 104 anchors, BatchNorm in training mode — one
    forward + backward of the HIP path against the REFERENCE's own run (golden G15, oracle/gen_golden_curves.py g15, fp32 and
    fp64): loss and its two parts, per-pyramid-level activation checksums, strided activation samples, every parameter's
    gradient norm, 1024-element gradient slices.  Criterion: |hip - f64| <= 3 |ref32 - f64| + 1e-3 |f64|."""
    g = load_golden('g15_retinanet_bs16')
    net, lf = _g15_net_and_loss(g)
    x, y = _g15_batch(g, 1500)
    anchors, reg, clas = net(x)
    loss = lf([anchors, reg, clas], y)
    loss.backward()
    assert anchors.shape[0] == 49104 and reg.shape == (16, 49104, 4) and clas.shape == (16, 49104, 20)
    got = torch.stack([loss.detach(), torch.as_tensor(float(lf.reg_loss), device=DEV), torch.as_tensor(float(lf.clas_loss), device=DEV)])
    assert_within_reference_gap(got, g, 'a.loss', 'loss / reg_loss / clas_loss')
    r, c = reg.detach().double(), clas.detach().double()
    o, lv = 0, []
    for l in range(3, 8):
        n_l = (512 // 2 ** l) ** 2 * 9
        lv.append(torch.stack([r[:, o:o + n_l].sum(), r[:, o:o + n_l].abs().sum(), c[:, o:o + n_l].sum(), (c[:, o:o + n_l] ** 2).sum()]))
        o += n_l
    lv = torch.stack(lv)
    r32, r64 = g['a.level_sums.f32'], g['a.level_sums.f64']
    # checksums: sums of ~1e6 terms; the plain `reg` sum cancels (|sum| << sum |.|), so its scale is the |.|-sum next to it
    scale = np.stack([r64[:, 1], r64[:, 1], np.abs(r64[:, 2]), r64[:, 3]], 1)
    err, gap = np.abs(lv.cpu().numpy() - r64), np.abs(r32 - r64)
    assert (err <= 3 * gap + 1e-4 * scale).all(), 'per-level activation checksums: worst err/scale %.2e' % (err / scale).max()
    assert_within_reference_gap(r.reshape(-1)[::397], g, 'a.reg_sample', 'reg activations (every 397th)')
    assert_within_reference_gap(c.reshape(-1)[::1987], g, 'a.clas_sample', 'clas activations (every 1987th)')
    n32, n64 = g['a.grad_norms.f32'], g['a.grad_norms.f64']
    names = [str(s) for s in g['param_names']]
    hip = np.array([0.0 if p.grad is None else p.grad.double().norm().item() for _, p in net.named_parameters()])
    bad = ['%s: hip %.6e ref32 %.6e f64 %.6e' % (n, h, a, b) for n, h, a, b in zip(names, hip, n32, n64)
           if not abs(h - b) <= 3 * abs(a - b) + 1e-3 * abs(b)]
    print('gradient norms: worst rel |hip-f64| %.2e, worst rel |ref32-f64| %.2e' % (
        (np.abs(hip - n64) / np.maximum(n64, 1e-300)).max(), (np.abs(n32 - n64) / np.maximum(n64, 1e-300)).max()))
    assert not bad, '%d gradient norms outside 3x the reference gap + 1e-3:\n%s' % (len(bad), '\n'.join(bad))
    sd = dict(net.named_parameters())
    for n in [str(s) for s in g['slice_names']]:
        if 'a.grad.%s.f32' % n in g:
            gr = sd[n].grad
            assert_within_reference_gap(gr.contiguous().reshape(-1)[:1024], g, 'a.grad.' + n, 'gradient slice ' + n, normwise=True)


@pytest.mark.gpu
def test_g15_retinanet_10_step_loss_curve_every_step_within_1e3():
    """VERDICT r2 next #1(a), RetinaNet leg: 10 consecutive `train1minibatch` steps (SGD momentum 0.9, lr [1e-4, 3e-4, 1e-3], wd 1e-4,
    10 distinct batches of 16 images with 1-8 boxes each) at 512 x 512 against the REFERENCE's own Learner (golden G15; its fp32 and
    fp64 runs stay within 3e-4 on every step): |hip - ref32| <= 1e-3 |ref32| on EVERY step."""
    from neuralnetworklibrary_amd.General.Learner import Learner
    g = load_golden('g15_retinanet_bs16')
    r32, r64 = g['losses.f32'], g['losses.f64']
    assert (np.abs(r32 - r64) / np.abs(r64)).max() < 3e-4
    net, lf = _g15_net_and_loss(g)

    class D:
        bs, target_type = int(g['N']), 'bbox'
    d = D(); d.train_dl = [(None, [torch.zeros(16)])]; d.val_dl = d.train_dl
    learner = Learner('/tmp/nnl_test_g15', d, net, optimizer='SGD_Mom', loss_func=lf)
    learner.init_optimizer(wd=float(g['wd']))
    lr = [float(v) for v in g['lr']]
    losses = []
    for i in range(int(g['steps'])):
        x, y = _g15_batch(g, 1501 + i)
        losses.append(learner.train1minibatch(x, y, lr))
    losses = np.array(losses)
    rel32 = np.abs(losses - r32) / np.abs(r32)
    print('losses         ', np.array2string(losses, precision=5))
    print('rel |hip-ref32|', np.array2string(rel32, precision=1))
    print('rel |ref32-f64|', np.array2string(np.abs(r32 - r64) / np.abs(r64), precision=1))
    assert (rel32 <= 1e-3).all(), 'step losses off the reference fp32 curve: worst %.2e at step %d' % (rel32.max(), rel32.argmax())
    abs_sums = np.array([p.double().abs().sum().item() for _, p in net.named_parameters()])
    a32, a64 = g['after.abs_sums.f32'], g['after.abs_sums.f64']
    tol = 3 * np.abs(a32 - a64) + 1e-3 * np.abs(a64) + 1e-6          # as far from fp64 as the reference's own fp32 run (x3) + 1e-3
    bad = np.nonzero(np.abs(abs_sums - a64) > tol)[0]
    assert len(bad) == 0, '%d parameter |.|-sums outside 3x the reference fp32/fp64 gap + 1e-3: %s' % (
        len(bad), [(str(g['param_names'][i]), abs_sums[i], a32[i], a64[i]) for i in bad[:5]])
