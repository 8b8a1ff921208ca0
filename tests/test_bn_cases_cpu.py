"""tests/bn_cases.py without a GPU: every case reaches the launch regime it names (through nnl_debug_bn_plan, which calls the planner
functions of csrc/batchnorm.hip themselves), no regime is left without a case, the fp64 reference agrees with torch's BatchNorm under
autograd, and the int-mode comparisons of tests/test_bn_abi_gpu.py notice a single row dropped from or added to a reduction."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bn_cases as bc


def plan(rows, C, N=0, H=0, W=0, P=0, Q=0):
    from neuralnetworklibrary_amd._lib import lib
    out = (ctypes.c_int32 * 10)(*([-7] * 10))
    assert lib.nnl_debug_bn_plan(rows, C, N, H, W, P, Q, out) == 1
    return list(out)


@pytest.mark.parametrize('case', bc.CASES, ids=bc.case_id)
def test_case_reaches_its_regimes(case):
    p = plan(case.rows, case.C)
    f = bc.facts(case.rows, case.C, p)
    assert f.VEC == (4 if case.C % 4 == 0 else 1) and f.rpb * f.L == 256 and f.gy == bc.cdiv(f.CG, f.L)
    assert f.gx * f.gy <= f.cap and (f.ew_blocks * 256) % f.CG == 0
    assert case.regimes, 'a case names the regime it exists for'
    for name in case.regimes:
        assert bc.REGIMES[name](f), '%s does not reach "%s": plan %s, %s' % (bc.case_id(case), name, p, f)


def test_census_every_regime_has_a_case():
    claimed = {name for c in bc.CASES for name in c.regimes}
    assert claimed == set(bc.REGIMES), 'regimes without a case: %s' % sorted(set(bc.REGIMES) - claimed)
    assert len({(c.rows, c.C) for c in bc.CASES}) == len(bc.CASES)
    assert max(c.rows for c in bc.CASES) <= bc.INT_MAX_ROWS


def test_plan_query_edges():
    from neuralnetworklibrary_amd._lib import lib
    out = (ctypes.c_int32 * 10)(*([-7] * 10))
    for rows, C in ((0, 4), (4, 0), (-1, 4), (4, 1 << 24)):
        assert lib.nnl_debug_bn_plan(rows, C, 0, 0, 0, 0, 0, out) == 0 and list(out) == [-7] * 10
    assert lib.nnl_debug_bn_plan(4, 4, 0, 0, 0, 0, 0, None) == 0
    assert plan(64, 64)[8:] == [-1, -1]                                   # no stem geometry given
    # the production shape of the issue: ResNet-34, 64 images, 56 x 56 x 64 -> capped, 3 unrolled passes of the 4-way loop
    f = bc.facts(200704, 64, plan(200704, 64))
    assert f.capped and f.gx == 1024 and {k // 4 for k in f.k_set} == {3}


def test_stem_cases_and_grids():
    from neuralnetworklibrary_amd._lib import lib
    grids = []
    for N, H, W, C, ks, st, pd in bc.STEM_CASES:
        assert H % 2 == 1 and W % 2 == 1 and lib.nnl_bn_relu_maxpool_supported(C) == 1
        P, Q = bc.pool_out(H, ks, st, pd), bc.pool_out(W, ks, st, pd)
        p = plan(N * H * W, C, N, H, W, P, Q)
        assert p[8] == min(1024, max(1, bc.cdiv(N * H * W * C // 4, 4096))) and p[9] == min(1024, max(1, bc.cdiv(N * P * Q * C // 4, 4096)))
        grids.append(p[8])
    assert {c[4:] for c in bc.STEM_CASES} == set(bc.STEM_GEOMS) and {c[3] for c in bc.STEM_CASES} == {4, 16, 64, 1024}
    assert max(grids) == 1024 and min(grids) == 1, 'one stem case reaches the capped bnpool_grid'
    assert plan(64, bc.STEM_REFUSED_C, 1, 8, 8, 4, 4)[8:] == [-1, -1]


def test_stem_refuses_c12_on_the_host():
    """the check precedes every pointer check and every launch: NULL pointers, no GPU"""
    from neuralnetworklibrary_amd._lib import lib
    assert lib.nnl_bn_relu_maxpool_supported(bc.STEM_REFUSED_C) == 0
    st = lib.nnl_bn_relu_maxpool_fwd(None, None, None, None, None, None, None, None, None, None, None, 2, 15, 13, bc.STEM_REFUSED_C, 8, 7,
                                     3, 2, 1, bc.EPS, bc.MOMENTUM, 1, None, None, 0, None)
    assert st == -1 and bc.STEM_REFUSAL in lib.nnl_last_error() and b'C=12' in lib.nnl_last_error()
    st = lib.nnl_bn_relu_maxpool_bwd(None, None, None, None, None, None, None, None, None, None, None, None, None, 2, 15, 13,
                                     bc.STEM_REFUSED_C, 8, 7, 3, 2, 1, 1, None, 0, None)
    assert st == -1 and bc.STEM_REFUSAL in lib.nnl_last_error()


def test_ext_cases_cover_both_finalize_widths():
    tiles = sorted({t for t, _ in bc.EXT_CASES})
    assert tiles == [1, 63, 98, 1023, 1024, 1793, 3136] and {C for _, C in bc.EXT_CASES} == {6, 64}
    assert bc.ext_rows_of(1) == 64 and bc.ext_rows_of(1024) == 1023 * 64 + 1 and bc.ext_rows_of(3136) <= bc.INT_MAX_ROWS


# ---- the reference against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('case', bc.SMALL, ids=bc.case_id)
def test_reference_agrees_with_torch_autograd(case, relu, training):
    if training and case.rows == 1:
        with pytest.raises(ValueError):                            # torch refuses one value per channel; the header defines it (variance 0)
            F.batch_norm(torch.zeros(1, case.C), None, None, training=True)
        return
    d = {k: v.double() for k, v in bc.make_data(case.rows, case.C, 'randn', 3.0, seed=1).items()}
    x, res = d['x'].clone().requires_grad_(True), d['res'].clone().requires_grad_(True)
    gamma, beta = d['gamma'].clone().requires_grad_(True), d['beta'].clone().requires_grad_(True)
    rm, rv = d['rmean'].clone(), d['rvar'].clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, training, bc.MOMENTUM, bc.EPS) + res
    y = torch.relu(y) if relu else y
    y.backward(d['dy'])

    n = case.rows
    mean, var = bc.batch_stats(d['x']) if training else (d['rmean'], d['rvar'])
    yr, invstd = bc.bn_fwd_ref(d['x'], d['gamma'], d['beta'], d['res'], mean, var, bc.EPS, relu)
    b = bc.bn_bwd_ref(d['dy'], (yr > 0).double() if relu else None, d['x'], d['gamma'], mean, invstd, training)
    tol = dict(rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(yr, y.detach(), **tol)
    torch.testing.assert_close(b['dx'], x.grad, **tol)
    torch.testing.assert_close(b['dres'], res.grad, **tol)
    torch.testing.assert_close(b['dgamma'], gamma.grad, **tol)
    torch.testing.assert_close(b['dbeta'], beta.grad, **tol)
    if training:
        torch.testing.assert_close(bc.running_update(d['rmean'], mean, bc.MOMENTUM), rm, **tol)
        torch.testing.assert_close(bc.running_update(d['rvar'], bc.unbiased(var, n), bc.MOMENTUM), rv, **tol)
    else:
        assert torch.equal(rm, d['rmean']) and torch.equal(rv, d['rvar'])


def test_reference_without_affine_matches_torch():
    d = {k: v.double() for k, v in bc.make_data(33, 7, 'randn', 0.0, seed=2).items()}
    x = d['x'].clone().requires_grad_(True)
    y = F.batch_norm(x, None, None, None, None, True, 0.0, bc.EPS)
    y.backward(d['dy'])
    mean, var = bc.batch_stats(d['x'])
    yr, invstd = bc.bn_fwd_ref(d['x'], None, None, None, mean, var, bc.EPS, False)
    torch.testing.assert_close(yr, y.detach(), rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(bc.bn_bwd_ref(d['dy'], None, d['x'], None, mean, invstd, True)['dx'], x.grad, rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize('case', bc.SMALL + [bc.CASES[7]], ids=bc.case_id)
def test_sums_form_equals_the_definition(case):
    """the header's shifted-sums expression and the plain definition are the same numbers in fp64, in both data modes"""
    for mode, off in (('int', 0.0), ('randn', 40.0)):
        d = bc.make_data(case.rows, case.C, mode, off, seed=3)
        x = d['x'].double()
        S1, S2 = bc.shifted_sums(x, x[0])
        s = bc.stats_from_sums(S1, S2, x[0], float(case.rows), d['rmean'].double(), d['rvar'].double(), bc.MOMENTUM, bc.EPS)
        mean, var = bc.batch_stats(x)
        torch.testing.assert_close(s['mean'], mean, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(s['var'], var, rtol=1e-9, atol=1e-11)
        torch.testing.assert_close(s['rvar'], bc.running_update(d['rvar'].double(), bc.unbiased(var, case.rows), bc.MOMENTUM), rtol=1e-9, atol=1e-11)
        if mode == 'int':
            assert float(S2.max()) <= 64 * case.rows < 2 ** 24 and torch.equal(S1, S1.round())


def test_stem_reference_matches_torch_autograd():
    """relu(bn(x)) pooled, forward and backward, against autograd in fp64 (scale / shift given in fp64-exact fp32 values: no ties)"""
    N, H, W, C, ks, st, pd = 2, 9, 7, 8, 3, 2, 1
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, W, C, generator=g)
    gamma, beta = torch.linspace(0.5, 1.5, C), torch.linspace(-0.4, 0.4, C)
    gamma[:3] = torch.tensor([1e-3, 0.0, -0.7])
    xd = x.double()
    mean, var = bc.batch_stats(xd.view(-1, C))
    invstd = 1.0 / torch.sqrt(var + bc.EPS)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    z, y, idx = bc.stem_forward_fp32(xd, scale, shift, ks, st, pd)                 # (fp64 here: the function is dtype-agnostic)
    xa = xd.clone().requires_grad_(True)
    ya = F.max_pool2d(torch.relu(F.batch_norm(xa.permute(0, 3, 1, 2), None, None, gamma.double(), beta.double(), True, 0.0, bc.EPS)),
                      ks, st, pd).permute(0, 2, 3, 1)
    dpool = torch.randn(ya.shape, generator=g).double()
    ya.backward(dpool)
    torch.testing.assert_close(y, ya.detach(), rtol=1e-9, atol=1e-9)
    gin = bc.stem_scatter(dpool, idx, z, H, W, ks, st, pd)
    b = bc.bn_bwd_ref(gin.view(-1, C), None, xd.view(-1, C), gamma.double(), mean, invstd, True)
    torch.testing.assert_close(b['dx'].view(N, H, W, C), xa.grad, rtol=1e-8, atol=1e-9)


# ---- the int-mode comparisons notice one row ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['dropped', 'added'])
@pytest.mark.parametrize('case', [bc.CASES[4], bc.CASES[9], bc.CASES[13], bc.CASES[16]], ids=bc.case_id)
def test_int_mode_notices_one_row(case, what):
    """A reduction that skips one row, or takes it twice, still divides by rows.  Its results, rounded to fp32 as a kernel would return
    them, must fail the bit-exact dbeta comparison and the derived-bound save_mean comparison of the GPU sweep — and the honest sums,
    evaluated in fp32 operation by operation as bn_finalize_kernel does, must pass them (so the bound is neither too tight nor too wide)."""
    rows, C = case.rows, case.C
    d = bc.make_data(rows, C, 'int', seed=4)
    x, dy = d['x'].double(), d['dy'].double()
    gate = (d['res'] > 0).double()                                              # any gate: the GPU test takes it from the kernel's y
    g = dy * gate
    n = float(rows)
    S1, S2 = bc.shifted_sums(x, x[0])
    want = bc.stats_from_sums(S1, S2, x[0], n, d['rmean'].double(), d['rvar'].double())
    dbeta = g.sum(0)

    # the kernel's arithmetic in fp32, operation by operation
    f = lambda t: t.float()
    q32 = f(S1) / f(torch.tensor(n))
    m32 = f(x[0]) + q32
    v32 = torch.clamp((f(S2) - f(S1) * q32) / f(torch.tensor(n)), min=0)
    is32 = 1.0 / torch.sqrt(v32 + torch.tensor(bc.EPS, dtype=torch.float32))
    assert bc.within(m32, want['mean'], want['mean_bound']), bc.worst(m32, want['mean'], want['mean_bound'])
    assert bc.within(is32, want['invstd'], want['invstd_bound']), bc.worst(is32, want['invstd'], want['invstd_bound'])
    assert torch.equal(f(dbeta).double(), dbeta)

    r = next(i for i in range(1, rows) if bool((x[i] != x[0]).any()) and bool((g[i] != 0).any()))
    sign = -1.0 if what == 'dropped' else 1.0
    dr = x[r] - x[0]
    bad = bc.stats_from_sums(S1 + sign * dr, S2 + sign * dr * dr, x[0], n)
    bad_mean, bad_invstd, bad_dbeta = bad['mean'].float(), bad['invstd'].float(), (dbeta + sign * g[r]).float()
    assert not torch.equal(bad_dbeta, dbeta.float()), 'bit-exact dbeta does not notice the row'
    assert not bc.within(bad_mean, want['mean'], want['mean_bound']), 'save_mean within its bound although one row was %s' % what
    assert not bc.within(bad_invstd, want['invstd'], want['invstd_bound']), 'save_invstd within its bound although one row was %s' % what
