"""Squeeze-excite kernels (csrc/se.hip) and ceil-mode max pooling against fp64 torch on the CPU.

  out = relu( x * sigmoid(fc2(relu(fc1(mean_hw(x))))) + residual )

The scaling pass and its backward are checked at the C entry points, where z (the pre-sigmoid logits) is an input, so that the bounds
are those of the pass alone (u = 2^-24):
  forward   |err| <= 16 u (|x| + |residual|) elementwise: one multiply-add plus a sigmoid from an exponential and a division, each
            within a few ulp;
  dx, dres  |err| <= 16 u |dy| elementwise.  dx = g sigmoid(z) and dres = g have |dy| as their only operand of magnitude — x and the
            residual do not enter them — so the forward's 16 u is taken per unit of |dy|; (a bound that also carried the factor
            |x| + |residual| would refuse the correctly rounded result wherever that sum is small);
  dz        |err| <= HW u sigmoid'(z) sum_h |g x|.
Elements whose fp64 pre-activation lies within 1e-4 of the ReLU step are left out of the backward comparison (two correct fp32
kernels may gate them differently): dy is zero there, so they do not enter dz either; their share is asserted to be at most 1 % on
the fp64 reference first (standard-normal x and residual: the density of the pre-activation at 0 is at most 0.4, expected share
below 1e-4).
The FC stage and the whole ops.se_excite are checked under the tolerance ops.linear's tests use (rtol 1e-4, atol 1e-5 max|ref|), with
dy zero within 1e-3 of the ReLU step (there the logits come out of two fp32 GEMMs).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

U = 2.0 ** -24
CASES = [(3, 7, 7, 64, 16), (2, 1, 1, 256, 16), (2, 5, 3, 20, 4), (1, 14, 14, 2048, 16)]        # N, H, W, C, r


def cid(c):
    return 'n%d-%dx%d-c%d-r%d' % c


def make(c, residual, seed=0):
    N, H, W, C, r = c
    g = torch.Generator().manual_seed(7000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()       # noqa: E731  (exact in fp32)
    d = dict(x=rn(N, H * W, C), z=rn(N, C), dy=rn(N, H * W, C), res=rn(N, H * W, C) if residual else None,
             w1=rn(C // r, C) / C ** 0.5, b1=rn(C // r) * 0.1, w2=rn(C, C // r) / (C // r) ** 0.5, b2=rn(C) * 0.1)
    return {k: (None if v is None else v.float().double()) for k, v in d.items()}


def ref_scale(d):
    "fp64 reference of the scaling pass with z given: out, pre, and the gradients for d['dy']"
    x, z = d['x'].clone().requires_grad_(True), d['z'].clone().requires_grad_(True)
    res = None if d['res'] is None else d['res'].clone().requires_grad_(True)
    pre = x * torch.sigmoid(z)[:, None, :] + (0 if res is None else res)
    out = torch.relu(pre)
    out.backward(d['dy'])
    return dict(out=out.detach(), pre=pre.detach(), dx=x.grad, dz=z.grad, dres=None if res is None else res.grad)


def dev32(t):
    return None if t is None else t.float().cuda().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('residual', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('c', CASES, ids=cid)
def test_excite_pass_fwd_bwd(c, residual):
    from neuralnetworklibrary_amd._lib import lib, check, ptr, stream
    N, H, W, C, r = c
    HW = H * W
    d = make(c, residual)
    pre = ref_scale(d)['pre']
    near = pre.abs() < 1e-4
    share = near.double().mean().item()
    print('share of pre-activations within 1e-4 of the ReLU step: %.2e' % share)
    assert share <= 0.01
    d['dy'] = d['dy'] * ~near
    ref = ref_scale(d)
    x, z, res, dy = dev32(d['x']), dev32(d['z']), dev32(d['res']), dev32(d['dy'])
    outs = []
    for _ in range(2):
        out, dx, dz = torch.empty_like(x), torch.empty_like(x), torch.empty_like(z)
        dres = torch.empty_like(x) if residual else None
        check(lib.nnl_se_excite_fwd(ptr(x), ptr(z), ptr(res), ptr(out), N, HW, C, stream()))
        check(lib.nnl_se_excite_bwd(ptr(dy), ptr(out), ptr(x), ptr(z), ptr(dx), ptr(dres), ptr(dz), N, HW, C, stream()))
        outs.append((out, dx, dz, dres))
    for a, b in zip(*outs):
        assert (a is None and b is None) or torch.equal(a, b), 'two calls differ'
    out, dx, dz, dres = [None if t is None else t.cpu().double() for t in outs[0]]
    d32 = d                                                # (make() returns fp32-representable values: the kernels saw exactly these)
    keep = ~(ref['pre'].abs() < 1e-4)
    mag = d32['x'].abs() + (0 if d32['res'] is None else d32['res'].abs())
    err = (out - ref['out']).abs()
    print('fwd: max err / bound = %.3f' % (err / (16 * U * mag)).max().item())
    assert bool((err <= 16 * U * mag).all())
    bound = 16 * U * d32['dy'].abs()
    for name, got in (('dx', dx), ('dres', dres)):
        if got is None:
            continue
        e = (got - ref[name]).abs()
        print('%s: max err / bound = %.3f' % (name, (e[keep] / bound[keep].clamp_min(1e-300)).max().item()))
        assert bool((e[keep] <= bound[keep]).all()), name
    s = torch.sigmoid(d32['z'])
    gated = d32['dy'] * (ref['pre'] > 0)
    zb = HW * U * (s * (1 - s)) * (gated * d32['x']).abs().sum(1)
    e = (dz - ref['dz']).abs()
    print('dz: max err / bound = %.3f' % (e / zb.clamp_min(1e-300)).max().item())
    assert bool((e <= zb).all())


def close(got, ref, msg):
    "the tolerance of ops.linear's tests (tests/test_conv_gpu.py): rtol 1e-4, atol 1e-5 max|ref| per tensor"
    assert_close(got, ref, rtol=1e-4, atol=1e-5 * ref.abs().max().item(), msg=msg)


@pytest.mark.gpu
@pytest.mark.parametrize('residual', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('c', CASES, ids=cid)
def test_se_excite_whole_and_fc_stage(c, residual):
    from neuralnetworklibrary_amd import ops
    from neuralnetworklibrary_amd._lib import lib, check, ptr, stream
    N, H, W, C, r = c
    d = make(c, residual, seed=1)
    # fp64 reference of the whole expression; dy is zero within 1e-3 of the ReLU step (here z comes out of two fp32 GEMMs)
    t = {k: (None if v is None else v.clone().requires_grad_(True)) for k, v in d.items() if k not in ('dy', 'z')}
    m_ref = t['x'].mean(1)
    z_ref = F.linear(torch.relu(F.linear(m_ref, t['w1'], t['b1'])), t['w2'], t['b2'])
    pre = t['x'] * torch.sigmoid(z_ref)[:, None, :] + (0 if t['res'] is None else t['res'])
    near = pre.detach().abs() < 1e-3
    assert near.double().mean().item() <= 0.01
    dy = d['dy'] * ~near
    ref_out = torch.relu(pre)
    ref_out.backward(dy)
    # the squeeze and the FC stage on their own
    x = dev32(d['x'])
    m = torch.empty(N, C, device='cuda')
    check(lib.nnl_se_squeeze(ptr(x), ptr(m), N, H * W, C, stream()))
    assert_close(m, m_ref.detach(), rtol=1e-5, atol=1e-6, msg='squeeze')
    w1, b1, w2, b2 = (dev32(d[k]) for k in ('w1', 'b1', 'w2', 'b2'))
    z = ops.linear(ops.linear(m, w1, b1, relu=True), w2, b2)
    close(z, F.linear(torch.relu(F.linear(m.cpu().double(), d['w1'], d['b1'])), d['w2'], d['b2']), 'fc stage')

    def logical(v):                                        # [N, HW, C] -> logical [N, C, H, W] over NHWC memory
        return v.view(N, H, W, C).permute(0, 3, 1, 2)

    def run():
        fc1, fc2 = torch.nn.Conv2d(C, C // r, 1).cuda(), torch.nn.Conv2d(C // r, C, 1).cuda()
        with torch.no_grad():
            fc1.weight.copy_(w1.view_as(fc1.weight))
            fc1.bias.copy_(b1)
            fc2.weight.copy_(w2.view_as(fc2.weight))
            fc2.bias.copy_(b2)
        xi = logical(x.clone()).requires_grad_(True)
        ri = logical(dev32(d['res'])).requires_grad_(True) if residual else None
        out = ops.se_excite(xi, fc1, fc2, ri)
        out.backward(logical(dev32(dy)))
        return [out.detach(), xi.grad, None if ri is None else ri.grad, fc1.weight.grad, fc1.bias.grad, fc2.weight.grad, fc2.bias.grad]
    a, b = run(), run()
    for p, q in zip(a, b):
        assert (p is None and q is None) or torch.equal(p, q), 'two calls differ'

    def rows(v):
        return v.permute(0, 2, 3, 1).reshape(N, H * W, C)
    close(rows(a[0]), ref_out.detach(), 'out')
    close(rows(a[1]), t['x'].grad, 'dx')
    if residual:
        close(rows(a[2]), t['res'].grad, 'dres')
    for got, k in ((a[3], 'w1'), (a[4], 'b1'), (a[5], 'w2'), (a[6], 'b2')):
        close(got.reshape(t[k].shape), t[k].grad, 'd' + k)


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', [(16, 14), (15, 17)])
def test_maxpool_ceil_mode(H, W):
    from neuralnetworklibrary_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-8, 9, (2, 8, H, W), generator=g).float()
    for pad in (0, 1):
        for ceil_mode in (True, False):
            xr = x.clone().requires_grad_(True)
            yr = F.max_pool2d(xr, 3, 2, pad, ceil_mode=ceil_mode)
            dy = torch.randint(-3, 4, yr.shape, generator=g).float()
            yr.backward(dy)
            xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
            y = ops.maxpool2d(xd, 3, 2, pad, ceil_mode=ceil_mode)
            y.backward(dy.cuda())
            assert y.shape == yr.shape
            assert torch.equal(y.cpu(), yr.detach()), 'values (pad %d ceil %s)' % (pad, ceil_mode)
            assert torch.equal(xd.grad.cpu(), xr.grad), 'gradient (pad %d ceil %s)' % (pad, ceil_mode)
    # distinct values: the arg-max is unique, so the gradient does not depend on the tie rule
    x = torch.randperm(2 * 8 * H * W, generator=g).float().view(2, 8, H, W)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 0, ceil_mode=True)
    dy = torch.randint(-3, 4, yr.shape, generator=g).float()
    yr.backward(dy)
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.maxpool2d(xd, 3, 2, 0, ceil_mode=True)
    y.backward(dy.cuda())
    assert torch.equal(y.cpu(), yr.detach()) and torch.equal(xd.grad.cpu(), xr.grad)
    from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipMaxPool2d
    assert HipMaxPool2d(3, stride=2, ceil_mode=True)(x.cuda()).shape == yr.shape
