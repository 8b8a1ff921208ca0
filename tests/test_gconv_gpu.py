"""Grouped convolution (csrc/gconv.hip through ops.grouped_conv2d) against torch.nn.functional.conv2d(groups=G) in fp64 on the CPU:
forward, dx, dw and db, at stride 1 and 2, with and without bias and the fused ReLU.

Two data modes, as in tests/conv_cases.py (whose constants and helpers are imported, the file is not edited):
  int    small integers: every product and partial sum is exact in fp32, so the kernels must reproduce the fp64 reference cast to fp32
         BIT FOR BIT — any indexing error shows without a tolerance;
  randn  weights scaled by 1/sqrt(Cg*R*R), the project's conv tolerance |err| <= ATOL_REL * max|ref| + RTOL * |ref|.
In randn mode with the ReLU epilogue, dy is zero wherever the fp64 pre-activation lies within 1e-4 of the ReLU step: two correct fp32
kernels may gate those outputs differently, and this way neither choice contributes.

The mutant tests (no GPU needed) show that the comparison notices a dropped tap, groups rotated by one and a mirrored dw.
"""
import collections
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc

GCase = collections.namedtuple('GCase', 'N G Cg Kg H W R')

CASES = [
    GCase(2, 64, 2, 4, 12, 10, 3),
    GCase(2, 32, 4, 4, 9, 7, 3),
    GCase(2, 32, 8, 8, 7, 7, 3),
    GCase(2, 64, 16, 32, 5, 9, 3),
    GCase(2, 32, 32, 32, 7, 7, 3),
    GCase(2, 3, 5, 7, 6, 11, 3),          # generic path: channel counts that are no multiples of 4
    GCase(2, 8, 1, 1, 8, 8, 3),           # depthwise
    GCase(2, 4, 4, 8, 8, 8, 1),           # R = 1
]
BIG = GCase(3, 32, 4, 4, 33, 31, 3)       # N*P*Q = 3069: the weight gradient runs in more than one slice of pixels
WIDE = GCase(2, 2, 40, 36, 9, 10, 3)      # more than 32 channels per group both ways: the operands come through the cache, not LDS


def gid(c):
    return 'n%d-g%d-cg%dkg%d-%dx%d-r%d' % c


def pad_of(c):
    return c.R // 2


def make(c, stride, mode, seed=0):
    "fp64 CPU tensors x [N,C,H,W], w [K,Cg,R,R], bias [K], dy [N,K,P,Q]"
    pad = pad_of(c)
    P, Q = cc.out_size(c.H, c.R, stride, pad), cc.out_size(c.W, c.R, stride, pad)
    g = torch.Generator().manual_seed(4000 + seed)
    shapes = dict(x=(c.N, c.G * c.Cg, c.H, c.W), w=(c.G * c.Kg, c.Cg, c.R, c.R), bias=(c.G * c.Kg,), dy=(c.N, c.G * c.Kg, P, Q))
    if mode == 'int':
        # |x|, |dy|, |bias| <= 2, |w| in {1, 2}: the largest sum is max(4 * Cg * R * R + 2, 4 * N * P * Q) < 2^24
        assert max(4 * c.Cg * c.R * c.R + 2, 4 * c.N * P * Q) < 1 << 24
        d = {k: torch.randint(-2, 3, s, generator=g).double() for k, s in shapes.items()}
        d['w'] = torch.randint(1, 3, shapes['w'], generator=g).double() * (torch.randint(0, 2, shapes['w'], generator=g).double() * 2 - 1)
    else:
        d = {k: torch.randn(s, generator=g, dtype=torch.float64) for k, s in shapes.items()}
        d['w'] = d['w'] / (c.Cg * c.R * c.R) ** 0.5
    return d


def reference(c, stride, d, bias, relu):
    x, w = d['x'].clone().requires_grad_(True), d['w'].clone().requires_grad_(True)
    b = d['bias'].clone().requires_grad_(True) if bias else None
    pre = F.conv2d(x, w, b, stride=stride, padding=pad_of(c), groups=c.G)
    y = torch.relu(pre) if relu else pre
    y.backward(d['dy'])
    return dict(y=y.detach(), pre=pre.detach(), dx=x.grad, dw=w.grad, db=b.grad if bias else None)


def differs(got, ref, mode):
    "None when `got` (fp32 or fp64) matches the fp64 reference under the mode's rule, else a description"
    got = got.detach().cpu()
    if mode == 'int':
        if torch.equal(got.float(), ref.float()):
            return None
        return '%d of %d elements differ bitwise' % ((got.float() != ref.float()).sum().item(), ref.numel())
    err = (got.double() - ref).abs()
    tol = cc.tolerance(ref)
    if bool((err <= tol).all()):
        return None
    return 'max err %.3e over tolerance by up to %.3e' % (err.max().item(), (err - tol).max().item())


def run_hip(c, stride, d, bias, relu, dev='cuda'):
    from neuralnetworklibrary_amd import ops
    x = d['x'].float().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = d['w'].float().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b = d['bias'].float().to(dev).requires_grad_(True) if bias else None
    y = ops.grouped_conv2d(x, w, b, stride, pad_of(c), c.G, relu=relu)
    y.backward(d['dy'].float().to(dev))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad if bias else None)


def check_case(c, stride, mode):
    for bias, relu in itertools.product((False, True), (False, True)):
        d = make(c, stride, mode)
        if relu and mode == 'randn':
            pre = reference(c, stride, d, bias, False)['pre']
            d['dy'] = d['dy'] * (pre.abs() > 1e-4)
        ref = reference(c, stride, d, bias, relu)
        got = run_hip(c, stride, d, bias, relu)
        assert got['y'].shape == ref['y'].shape
        for k in ('y', 'dx', 'dw') + (('db',) if bias else ()):
            bad = differs(got[k], ref[k], mode)
            assert bad is None, '%s stride %d %s bias=%s relu=%s: %s: %s' % (gid(c), stride, mode, bias, relu, k, bad)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['int', 'randn'])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c', CASES, ids=gid)
def test_grouped_conv_matches_fp64(c, stride, mode):
    check_case(c, stride, mode)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['int', 'randn'])
@pytest.mark.parametrize('c', [BIG, WIDE], ids=gid)
def test_grouped_conv_sliced_wgrad_and_wide_groups(c, mode):
    if c is BIG:
        from neuralnetworklibrary_amd._lib import lib
        assert lib.nnl_gconv2d_workspace_bytes(c.N, c.H, c.W, c.G * c.Cg, c.G * c.Kg, c.G, c.R, 1, 1) > 0, 'one slice only: not the case meant'
    for stride in (1, 2):
        check_case(c, stride, mode)


@pytest.mark.gpu
def test_grouped_conv_repeat_calls_give_the_same_bits():
    for c, stride in ((BIG, 1), (CASES[3], 2), (CASES[5], 1)):
        d = make(c, stride, 'randn')
        a, b = run_hip(c, stride, d, True, True), run_hip(c, stride, d, True, True)
        for k in ('y', 'dx', 'dw', 'db'):
            assert torch.equal(a[k], b[k]), '%s stride %d: %s differs between two calls' % (gid(c), stride, k)


@pytest.mark.gpu
def test_module_matches_nn_conv2d_state_and_output():
    "HipGroupedConv2d: nn.Conv2d's parameters and state_dict, weight stored channels_last, gradient in the parameter's layout"
    from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipGroupedConv2d
    torch.manual_seed(3)
    ref = torch.nn.Conv2d(32, 64, 3, stride=2, padding=1, groups=8).double()
    m = HipGroupedConv2d(32, 64, 3, stride=2, padding=1, groups=8)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    m = m.cuda()
    assert m.weight.is_contiguous(memory_format=torch.channels_last)
    x = torch.randn(2, 32, 9, 11, dtype=torch.float64)
    y = m(x.float().cuda())
    y.sum().backward()
    yr = ref(x)
    yr.sum().backward()
    assert differs(y, yr.detach(), 'randn') is None
    assert differs(m.weight.grad, ref.weight.grad, 'randn') is None and differs(m.bias.grad, ref.bias.grad, 'randn') is None
    assert m.weight.grad.stride() == m.weight.stride()


# ---- mutants: the comparison notices the bugs it is for (CPU only) ---------------------------------------------------------------
MUTANT_CASES = [(CASES[1], 1), (CASES[3], 2), (CASES[5], 1)]


@pytest.mark.parametrize('mode', ['int', 'randn'])
@pytest.mark.parametrize('c,stride', MUTANT_CASES, ids=lambda v: gid(v) if isinstance(v, GCase) else 's%d' % v)
def test_mutants_are_noticed(c, stride, mode):
    d = make(c, stride, mode)
    ref = reference(c, stride, d, False, False)
    pad, K = pad_of(c), c.G * c.Kg
    # a dropped tap: output pixel (0, 0) loses the first tap that falls inside the input
    y = ref['y'].clone()
    xg = d['x'][:, :, 0, 0].reshape(c.N, c.G, c.Cg)
    wg = d['w'][:, :, pad, pad].reshape(c.G, c.Kg, c.Cg)
    y[:, :, 0, 0] -= torch.einsum('ngc,gkc->ngk', xg, wg).reshape(c.N, K)
    assert differs(y, ref['y'], mode) is not None
    # groups rotated by one: every output group reads the next group's input channels
    y = F.conv2d(torch.roll(d['x'], -c.Cg, dims=1), d['w'], None, stride=stride, padding=pad, groups=c.G)
    assert differs(y, ref['y'], mode) is not None
    # dw with the (0, 0) filter slice swapped with its mirror
    geom = collections.namedtuple('RS', 'R S')(c.R, c.R)
    dw, _ = cc.mutant_mirrored_dw(geom, ref)
    assert differs(dw, ref['dw'], mode) is not None
    # and the reference itself, rounded to fp32, passes
    for k in ('y', 'dx', 'dw'):
        assert differs(ref[k].float(), ref[k], mode) is None
