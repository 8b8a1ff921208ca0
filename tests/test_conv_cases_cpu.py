"""What can be said about the conv C-ABI sweep without a device: the case list keeps its own conditions, int mode is exact by
construction, the fp64 reference notices the bugs the sweep is for, the planner-side queries agree with what the list marks, and the
three entry points validate their arguments before any HIP call."""
import ctypes

import pytest
import torch

import conv_cases as cc


def _geom(c, P=None, Q=None):
    from neuralnetworklibrary_amd import _lib
    p, q = cc.PQ(c)
    return _lib.ConvGeom(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad, p if P is None else P, q if Q is None else Q)


def test_the_list_keeps_its_conditions():
    from neuralnetworklibrary_amd._lib import lib
    assert len(cc.NAMED_BIG) <= 5
    total = 0.0
    for c in cc.CASES:
        P, Q = cc.PQ(c)
        assert cc.valid(c), cc.case_id(c)
        g = _geom(c)
        # check_geom runs first in every entry point; the null pointers after it are the only complaint left for a legal geometry
        st = lib.nnl_conv2d_fwd(None, None, None, None, ctypes.byref(g), 0, None, 0, None, None, None, None, None)
        assert st == -1 and b'null pointer' in lib.nnl_last_error(), (cc.case_id(c), lib.nnl_last_error())
        cap = cc.FLOP_CAP_NAMED if c.name in cc.NAMED_BIG else cc.FLOP_CAP
        assert cc.flop(c) <= cap, '%s: %.2e flop per pass' % (cc.case_id(c), cc.flop(c))
        assert c.N * c.H * c.W * c.C < cc.MAX_ELEMS and c.N * P * Q * c.K < cc.MAX_ELEMS, cc.case_id(c)
        total += cc.flop(c)
    assert total <= cc.FLOP_CAP_LIST, '%.2e flop per pass over the list' % total


def test_every_class_is_present():
    cs = cc.CASES
    count = lambda pred: sum(1 for c in cs if pred(c))                       # noqa: E731
    for f in cc.FILTERS + [(49, 1)]:
        for stride in ((1, 2, 3) if f != (49, 1) else (1,)):
            assert count(lambda c: (c.R, c.S) == f and c.stride == stride) >= 1, 'filter %s at stride %d' % (f, stride)
    big = lambda c: max(c.R, c.S)                                            # noqa: E731
    assert count(lambda c: c.pad == 0 and big(c) > 1) >= 12
    assert count(lambda c: c.pad == big(c) // 2 and big(c) > 1) >= 12
    assert count(lambda c: c.pad == big(c) - 1 and big(c) > 2) >= 12
    assert count(lambda c: c.pad >= c.R and c.pad >= c.S and c.R * c.S > 1) >= 2
    assert count(lambda c: c.R * c.S == 1 and c.pad == 1) >= 3
    assert count(lambda c: (c.N, c.C, c.H, c.W, c.K, c.R, c.S, c.stride, c.pad) == (1, 16, 4, 4, 16, 3, 3, 1, 130)) == 1
    assert count(lambda c: (c.N, c.C, c.H, c.W, c.K, c.R, c.S, c.stride, c.pad) == (1, 16, 4, 4, 16, 3, 3, 2, 260)) == 1
    s2 = [c for c in cs if c.stride == 2]
    assert sum(1 for c in s2 if c.H % 2 == 0 and c.W % 2 == 0) >= 5 and sum(1 for c in s2 if c.H % 2 == 1 or c.W % 2 == 1) >= 5
    assert count(lambda c: c.stride > 1 and ((c.H + 2 * c.pad - c.R) % c.stride != 0 or (c.W + 2 * c.pad - c.S) % c.stride != 0)) >= 10
    assert count(lambda c: c.H != c.W) >= 50
    for v in cc.SIZES:
        assert count(lambda c: v in (c.H, c.W)) >= 1, 'size %d' % v
    assert count(lambda c: 1 in cc.PQ(c)) >= 5
    assert count(lambda c: c.H < c.R or c.W < c.S) >= 5
    for v in cc.CHANNELS:
        assert count(lambda c: c.C == v) >= 1 and count(lambda c: c.K == v) >= 1, 'channels %d' % v
    for v in cc.BATCHES:
        assert count(lambda c: c.N == v) >= 3, 'batch %d' % v
    large = [c for c in cs if 50000 <= c.N * cc.PQ(c)[0] * cc.PQ(c)[1] <= 200000 and 64 <= c.K <= 256]
    assert len(large) >= 5, [cc.case_id(c) for c in large]
    assert count(lambda c: c.R * c.S > cc.IGEMM_MAX_TAPS) >= 3
    assert count(lambda c: (c.R, c.S) in ((1, 33), (1, 49)) and c.C % 16 == 0 and c.K % 16 == 0) >= 2     # the tap-table kernel on a raster wider than 32


@pytest.mark.parametrize('c', cc.CASES, ids=cc.case_id)
def test_int_mode_is_exact_by_construction(c):
    a, b, bound = cc.int_ranges(c)
    assert a >= 1 and b >= 1 and bound < 1 << 24
    if cc.flop(c) > 2e7:
        return                                                                # the bound is arithmetic; the data check below is for the small cases
    d = cc.make_data(c, 'int', seed=cc.CASES.index(c))
    assert d['w'].abs().min() >= 1 and d['w'].abs().max() <= b, 'no tap may be silently zero'
    for k in ('x', 'dy', 'bias', 'add_x'):
        assert d[k].abs().max() <= a and torch.equal(d[k], d[k].round())
    ref = cc.reference(c, d, addend=True)
    for k in ('y', 'dx', 'dw'):
        assert ref[k].abs().max() < bound and torch.equal(ref[k].float().double(), ref[k]), k


SAMPLE = [c for c in cc.CASES if c.name in ('pad0-3x3', 'pad2-3x3', 'pad1-1x1-s2', '4x4-s2-odd', '3x3-s2-tail', '1x33-pad', '7x7-s3', 'wino1d-forced-odd',
                                            'rowk-c180', 'Q-eq-1')] + \
         [cc._c('issue', 2, 64, 9, 7, 48, 3, 3, 1, 1, 'the case the issue quotes')] + [c for c in cc.GENERATED if cc.flop(c) < 5e7 and c.R * c.S > 1][::9]


@pytest.mark.parametrize('mode', ['int', 'randn'])
@pytest.mark.parametrize('c', SAMPLE, ids=cc.case_id)
def test_the_reference_notices_what_the_sweep_is_for(c, mode):
    """one border tap dropped at one output pixel, dx of one parity class zeroed, one (r, s) slice of dw swapped with its mirror: each mutant
    must differ from the reference — int mode: not equal; randn mode: by at least 10x the tolerance at the median affected element"""
    d = cc.make_data(c, mode, seed=3)
    ref = cc.reference(c, d)
    mutants = [('y', ref['pre'], cc.mutant_dropped_tap(c, d, ref)), ('dx', ref['dx'], cc.mutant_zeroed_parity_class(c, ref)),
               ('dw', ref['dw'], cc.mutant_mirrored_dw(c, ref))]
    ran = 0
    for name, good, m in mutants:
        if m is None:
            continue
        bad, where = m
        ran += 1
        if mode == 'int':
            assert not torch.equal(bad, good), name
        else:
            ratio = ((bad - good).abs() / cc.tolerance(good))[where]
            assert ratio.median().item() >= 10, '%s: the mutant is only %.1f x the tolerance at the median affected element' % (name, ratio.median().item())
    assert ran >= 1                                                       # (a 1x1 with pad 1 has neither a border tap at (0, 0) nor a mirror)


def test_relu_excluded_share_of_the_reference():
    """with the project's scaling the ReLU step excludes about 1e-4 of the outputs (|pre-activation| <= 1e-4): well under the 1 % the
    sweep allows"""
    for c in SAMPLE[:6]:
        d = cc.make_data(c, 'randn', seed=1)
        assert cc.relu_excluded_share(cc.reference(c, d)['pre']) < 0.01


def test_planner_queries_agree_with_what_the_list_marks(monkeypatch):
    from neuralnetworklibrary_amd._lib import lib
    seen = set()
    for c in cc.CASES:
        for k in ('NNL_CONV_WINO', 'NNL_WINO2_POS', 'NNL_WINO_PLAN_KS', 'NNL_WINO_PLAN_S', 'NNL_IGEMM_BALANCE', 'NNL_WGRAD_WINO', 'NNL_WGRAD_WINO2D'):
            monkeypatch.delenv(k, raising=False)
        for k, v in c.env.items():
            monkeypatch.setenv(k, v)
        lib.nnl_reload_env()
        g = _geom(c)
        pf, pd = lib.nnl_conv2d_wino_preferred(ctypes.byref(g), 0), lib.nnl_conv2d_wino_preferred(ctypes.byref(g), 1)
        wf, wd = lib.nnl_conv2d_fwd_workspace_bytes(ctypes.byref(g)), lib.nnl_conv2d_dgrad_workspace_bytes(ctypes.byref(g))
        if not (c.R == 3 and c.S == 3 and c.stride == 1 and c.pad == 1):
            assert pf == 0 and pd == 0, cc.case_id(c)
        if c.name.startswith('wino1d'):
            assert pf == 1 and wf >= c.K * 12 * c.C * 4, cc.case_id(c)
        if c.name.startswith('wino2d'):
            assert pf == 2 and wf >= c.K * 16 * c.C * 4, cc.case_id(c)
        if c.name == 'wino-none':
            assert pf == 0 and pd == 0
        if c.name.startswith('bal-') and c.name != 'bal-off':
            assert wf > 0, cc.case_id(c)
        if c.name == 'bal-off':
            assert wf == 0 and wd == 0
        if c.name == 'ktail-bal':
            assert wd > 0                                                    # the dgrad (K = 1000, one tap) is sliced
        if c.stride != 1:
            assert wd == 0, cc.case_id(c)
        if c.name.startswith('wgrad-wino'):
            assert lib.nnl_conv2d_wgrad_workspace_bytes(ctypes.byref(g)) >= (0 if c.name == 'wgrad-wino-off' else c.K * 12 * c.C * 4)
        seen.update((pf, pd))
    assert seen == {0, 1, 2}, 'nnl_conv2d_wino_preferred answers 0, 1 and 2 over the list'
    monkeypatch.undo()
    lib.nnl_reload_env()
    prefs = {(lib.nnl_conv2d_wino_preferred(ctypes.byref(_geom(c)), 0), lib.nnl_conv2d_wino_preferred(ctypes.byref(_geom(c)), 1))
             for c in cc.CASES if not c.env}
    assert {p for pq in prefs for p in pq} == {0, 1, 2}, 'under the default planner too: %s' % prefs


def test_route_notes_round_trip():
    from neuralnetworklibrary_amd._lib import lib
    buf = ctypes.create_string_buffer(64)
    assert lib.nnl_debug_route_record(1) == 0
    assert lib.nnl_debug_route_collect(buf, 64) == 0 and buf.value == b''
    c = cc.CASES[0]
    g = _geom(c)
    fake = ctypes.c_void_p(0x1000)
    # validation passes, the launch cannot happen without a device: the note of the decision is there all the same
    if not torch.cuda.is_available():
        st = lib.nnl_conv2d_fwd(fake, fake, None, fake, ctypes.byref(g), 0, None, 0, None, None, None, None, None)
        assert st == -2
        small = ctypes.create_string_buffer(4)
        assert lib.nnl_debug_route_collect(small, 4) == -1 and b'route_collect' in lib.nnl_last_error()
        assert lib.nnl_debug_route_collect(buf, 64) == 1 and buf.value == b'taps<64,64,16>;'
    assert lib.nnl_debug_route_collect(None, 0) == -1
    assert lib.nnl_debug_route_collect(buf, 64) == 0 and buf.value == b''
    assert lib.nnl_debug_route_record(0) == 0
    # off: nothing is recorded
    if not torch.cuda.is_available():
        lib.nnl_conv2d_fwd(fake, fake, None, fake, ctypes.byref(g), 0, None, 0, None, None, None, None, None)
    assert lib.nnl_debug_route_collect(buf, 64) == 0 and buf.value == b''


def _entry_points(lib, g, ptrs=True, relu=0):
    p = ctypes.c_void_p(0x1000) if ptrs else None
    gp = ctypes.byref(g) if g is not None else None
    return [('conv2d_fwd', lib.nnl_conv2d_fwd(p, p, None, p, gp, relu, None, 0, None, None, None, None, None)),
            ('conv2d_dgrad', lib.nnl_conv2d_dgrad(p, p, p, gp, None, None, 0, None, None)),
            ('conv2d_wgrad', lib.nnl_conv2d_wgrad(p, p, p, gp, None, 0, None))]


def _refused(g, status, text, sizes_zero=True):
    """all three entry points return `status` with `text` in nnl_last_error(), before any HIP call; the size queries answer 0"""
    from neuralnetworklibrary_amd._lib import lib
    p = ctypes.c_void_p(0x1000)
    gp = ctypes.byref(g)
    calls = [lambda: lib.nnl_conv2d_fwd(p, p, None, p, gp, 0, None, 0, None, None, None, None, None),
             lambda: lib.nnl_conv2d_dgrad(p, p, p, gp, None, None, 0, None, None),
             lambda: lib.nnl_conv2d_wgrad(p, p, p, gp, None, 0, None)]
    for call in calls:
        assert call() == status, lib.nnl_last_error()
        assert text in lib.nnl_last_error(), lib.nnl_last_error()
    if sizes_zero:
        assert lib.nnl_conv2d_fwd_workspace_bytes(gp) == 0 and lib.nnl_conv2d_dgrad_workspace_bytes(gp) == 0
        assert lib.nnl_conv2d_wgrad_workspace_bytes(gp) == 0


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_a_filter_larger_than_the_padded_input_is_refused(stride):
    """H + 2 pad < R: torch refuses the shape; C division would give P = (2 + 0 - 3) / 2 + 1 = 1 at stride >= 2"""
    from neuralnetworklibrary_amd import _lib
    for (H, W, R, S, pad) in ((2, 8, 3, 3, 0), (8, 2, 3, 3, 0), (1, 1, 5, 5, 1), (4, 4, 1, 7, 1)):
        for P, Q in ((1, 1), (0, 0), (1, (W + 2 * pad - S) // stride + 1), ((H + 2 * pad - R) // stride + 1, 1)):
            g = _lib.ConvGeom(2, H, W, 16, 16, R, S, stride, pad, P, Q)
            _refused(g, -1, b'larger than the padded input')
    with pytest.raises(RuntimeError):
        torch.nn.functional.conv2d(torch.zeros(1, 4, 2, 8), torch.zeros(4, 4, 3, 3), stride=stride)


def test_argument_validation_of_the_three_entry_points():
    from neuralnetworklibrary_amd import _lib
    lib = _lib.lib
    c = cc._c('v', 2, 16, 9, 7, 16, 3, 3, 2, 1, '')
    P, Q = cc.PQ(c)
    for dP, dQ in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        _refused(_geom(c, P + dP, Q + dQ), -1, b'do not match the geometry')
    _refused(_geom(c._replace(C=18)), -3, b'multiple of 4')
    _refused(_geom(c._replace(N=0)), -1, b'non-positive')
    _refused(_geom(c._replace(pad=-1), P, Q), -1, b'non-positive')
    g = _geom(c._replace(K=18))
    p = ctypes.c_void_p(0x1000)
    assert lib.nnl_conv2d_dgrad(p, p, p, ctypes.byref(g), None, None, 0, None, None) == -1 and b'K=18' in lib.nnl_last_error()
    assert lib.nnl_conv2d_wgrad(p, p, p, ctypes.byref(g), None, 0, None) == -1 and b'K=18' in lib.nnl_last_error()
    g = _geom(c)
    for relu in (-1, 3):
        assert lib.nnl_conv2d_fwd(p, p, None, p, ctypes.byref(g), relu, None, 0, None, None, None, None, None) == -1
        assert b'relu' in lib.nnl_last_error()
    for name, st in _entry_points(lib, g, ptrs=False):
        assert st == -1, name
        assert b'null pointer' in lib.nnl_last_error(), name
    for name, st in _entry_points(lib, None):
        assert st == -1, name
        assert b'null geometry' in lib.nnl_last_error(), name
    assert lib.nnl_conv2d_fwd_workspace_bytes(None) == 0 and lib.nnl_conv2d_dgrad_workspace_bytes(None) == 0
    assert lib.nnl_conv2d_wgrad_workspace_bytes(None) == 0
    # the fused addend where the header allows none: refused before any launch
    for cc_ in (c._replace(K=20), c._replace(stride=2, R=5, S=5, pad=2), c._replace(stride=1, R=9, S=9, pad=4)):
        g = _geom(cc_)
        assert lib.nnl_conv2d_dgrad(p, p, p, ctypes.byref(g), p, None, 0, None, None) == -3 and b'addend' in lib.nnl_last_error()
