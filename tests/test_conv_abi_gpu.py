"""The conv C ABI (nnl_conv2d_fwd / _dgrad / _wgrad, include/nnl.h) called directly over nn.Conv2d's geometry space, route by route.

Every case of tests/conv_cases.py runs in both data modes (`int`: bit-for-bit against the fp64 reference; `randn`: the project's
tolerance) and in every calling mode the header documents:
  ws+cnt  workspace of the size query and the persistent tile counters (what ops.py does)
  ws      workspace, tile_counters = NULL: split tiles are reduced by a second launch
  none    workspace = NULL
Each calling mode runs the forward with bias + activation and without either (the activation that goes with the bias alternates from
case to case; randn mode adds the sigmoid epilogue and, from 64 output pixels up, the BatchNorm partial sums), and the dgrad without and
with an addend (where the header allows none, the documented refusal is asserted), so every route meets every option.

Around every call: outputs and workspace sit inside larger allocations with sentinel bands, the output is pre-filled with NaN, the tile
counters must be zero again, the call is repeated and must reproduce itself bit for bit, and the library's route notes
(nnl_debug_route_record / _collect) go into the failure message and into a census that the tests at the end of the file check against
the list of launch routes read off csrc/conv2d.hip, csrc/wino.hip and csrc/wino2.hip.

Both modes run on every case: the file takes about half a minute on an MI355X, an eighth of the rest of the GPU suite.
"""
import collections
import ctypes
import sys

import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                                     # floats of sentinel on either side of an output / workspace
SENT = 12345.0
CALL_MODES = ('ws+cnt', 'ws', 'none')

CENSUS = collections.Counter()                   # (entry point, route) -> calls that reached it
OPTIONS = collections.defaultdict(set)           # (entry point, route) -> option labels it met
SWEPT = set()                                    # (case id, data mode) that ran in this process

_HAND = sorted(cc.HAND, key=cc.flop)                # small before large
SWEEP = [(c, 'int') for c in _HAND] + [(c, 'randn') for c in _HAND] + \
        [(c, 'int') for c in cc.GENERATED] + [(c, 'randn') for c in cc.GENERATED]


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


def _guarded(numel, fill):
    buf = torch.full((numel + 2 * GUARD,), SENT, device=DEV)
    view = buf[GUARD:GUARD + numel]
    view.fill_(fill)
    return buf, view


def _bands_intact(buf, numel):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + numel:] == SENT).all())


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def _routes_of(lib, call):
    """(status, [route names], raw note string) of one library call"""
    buf = ctypes.create_string_buffer(16384)
    lib.nnl_debug_route_record(1)
    try:
        st = call()
        n = lib.nnl_debug_route_collect(buf, len(buf))
    finally:
        lib.nnl_debug_route_record(0)
    raw = buf.value.decode()
    names = [r for r in raw.split(';') if r]
    assert n == len(names), 'route buffer overflow: %d notes, %d names' % (n, len(names))
    return st, names, raw


def _note(entry, names, label):
    for r in names:
        key = (entry, r.split('@')[0])
        CENSUS[key] += 1
        OPTIONS[key].add(label)


def _compare(mode, got, ref64, what, ctx):
    """int: bit for bit against the fp64 reference cast to fp32; randn: the project's tolerance"""
    assert not torch.isnan(got).any(), '%s: %d elements of %s were never written (NaN sentinel)' % (ctx, int(torch.isnan(got).sum()), what)
    ref = ref64.to(DEV)
    if mode == 'int':
        ref32 = ref.float()
        assert torch.equal(ref32.double(), ref), '%s: the reference of %s is not exact in fp32' % (ctx, what)
        if not torch.equal(got, ref32):
            bad = (got != ref32).nonzero()
            i = tuple(bad[0].tolist())
            raise AssertionError('%s: %s differs from the fp64 reference at %d of %d elements, first at %s: got %r, want %r' %
                                 (ctx, what, bad.shape[0], got.numel(), i, got[i].item(), ref32[i].item()))
    else:
        err = (got.double() - ref).abs()
        tol = cc.ATOL_REL * ref.abs().max() + cc.RTOL * ref.abs()
        if not bool((err <= tol).all()):
            i = tuple(int(v) for v in torch.unravel_index((err - tol).argmax(), err.shape))
            raise AssertionError('%s: %s max abs err %.3e at %s (got %r, want %r), tolerance there %.3e' %
                                 (ctx, what, err.max().item(), i, got[i].item(), ref[i].item(), tol[i].item()))


def _addend_allowed(c):
    """include/nnl.h: K % 16 == 0 (the tap-table kernel: at most 49 taps, tap offsets within its table) and stride 1, or a 3x3 / pad 1
    filter at stride 2"""
    if c.K % 16 != 0 or c.R * c.S > cc.IGEMM_MAX_TAPS:
        return False
    if c.stride == 1:
        return c.S <= 32 or c.pad <= 127
    return c.stride == 2 and c.R == 3 and c.S == 3 and c.pad == 1


@pytest.mark.parametrize('case,mode', SWEEP, ids=['%s-%s' % (cc.case_id(c), m) for c, m in SWEEP])
def test_sweep(case, mode, monkeypatch):
    from neuralnetworklibrary_amd import _lib, ops
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    c = case
    idx = cc.CASES.index(c)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    lib.nnl_reload_env()
    P, Q = cc.PQ(c)
    M = c.N * P * Q
    geom = _lib.ConvGeom(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad, P, Q)
    g = ctypes.byref(geom)
    cid = '%s [%s]' % (cc.case_id(c), mode)
    _say('case', cid)

    d = cc.make_data(c, mode, seed=idx)
    ref = cc.reference(c, d, bias=True, act=0, addend=False)
    ref_nobias = ref['pre'] - d['bias'].view(1, -1, 1, 1)
    x, dy = _nhwc(d['x']), _nhwc(d['dy'])
    w = d['w'].permute(0, 2, 3, 1).contiguous().float().to(DEV)               # KRSC
    bias, add_x = d['bias'].float().to(DEV), _nhwc(d['add_x'])
    pivot = d['pivot'].float().to(DEV)
    wt = torch.empty(c.C, c.R, c.S, c.K, device=DEV)
    assert lib.nnl_conv2d_weight_transpose(ptr(w), ptr(wt), c.K, c.R, c.S, c.C, stream()) == 0
    assert torch.equal(wt, w.permute(3, 1, 2, 0).contiguous()), 'nnl_conv2d_weight_transpose'
    counters = ops._tile_counters(x.device)
    pre_nhwc = {True: ref['pre'].permute(0, 2, 3, 1).contiguous(), False: ref_nobias.permute(0, 2, 3, 1).contiguous()}
    dx_ref = ref['dx'].permute(0, 2, 3, 1).contiguous()
    dw_ref = ref['dw'].permute(0, 2, 3, 1).contiguous()

    def act_ref(t, act):
        return torch.relu(t) if act == 1 else torch.sigmoid(t) if act == 2 else t

    def guarded_call(entry, label, out_numel, out_shape, wsb, call_mode, make_call, accept=(0,)):
        """runs make_call(out, ws, wsb, counters) twice inside guard bands; returns (status, output of the first run, routes)"""
        ws_buf = ws = None
        if call_mode != 'none' and wsb > 0:
            ws_buf, ws = _guarded(wsb // 4 + 4, float('nan'))
        elif call_mode != 'none':
            ws_buf, ws = _guarded(4, float('nan'))                             # a workspace pointer with a size of zero bytes
        cnt = counters if call_mode == 'ws+cnt' else None
        outs = []
        for rep in range(2):
            out_buf, out = _guarded(out_numel, float('nan'))
            _say('  call', entry, label, call_mode, 'run', rep)
            st, names, raw = _routes_of(lib, lambda: make_call(out, ws, wsb if ws is not None else 0, cnt))
            torch.cuda.synchronize()
            ctx = '%s %s %s %s routes=%s' % (cid, entry, label, call_mode, raw)
            _say('  routes', raw, 'status', st)
            assert st in accept, '%s: status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
            if st != 0:
                return st, None, names, ctx
            assert _bands_intact(out_buf, out_numel), '%s: wrote outside the output (guard band touched)' % ctx
            if ws_buf is not None:
                assert _bands_intact(ws_buf, ws.numel()), '%s: wrote outside the workspace (guard band touched)' % ctx
            assert int(counters.abs().sum()) == 0, '%s: tile counters not back to zero' % ctx
            if rep == 0:
                _note(entry, names, label + '|' + call_mode)
            outs.append(out.view(out_shape))
        assert torch.equal(outs[0], outs[1]) or bool(torch.isnan(outs[0]).any()), '%s: two runs differ (not bitwise reproducible)' % ctx
        return 0, outs[0], names, ctx

    # ---- forward ----------------------------------------------------------------------------------------------------------------
    wsb_f = lib.nnl_conv2d_fwd_workspace_bytes(g)
    act0 = (idx // 2) % 2                                                       # the activation that goes with the bias alternates
    variants = [(True, act0, mode == 'randn' and M >= 64), (False, 1 - act0, False)]
    if mode == 'randn':
        variants.append((True, 2, False))
    for call_mode in CALL_MODES:
        for has_bias, act, stats in variants:
            rows_max = (M + 63) // 64
            part = torch.zeros(rows_max * c.K * 2 + 8, device=DEV) if stats else None
            bn_rows = ctypes.c_int32(-1)
            label = 'bias=%d,act=%d,stats=%d' % (has_bias, act, stats)

            def fwd(out, ws, wsb, cnt):
                return lib.nnl_conv2d_fwd(ptr(x), ptr(w), ptr(bias) if has_bias else None, ptr(out), g, act, ptr(ws), wsb, ptr(cnt),
                                          ptr(part), ptr(pivot) if stats else None, ctypes.byref(bn_rows) if stats else None, stream())
            st, y, names, ctx = guarded_call('fwd', label, M * c.K, (c.N, P, Q, c.K), wsb_f, call_mode, fwd, accept=(0, -3) if act == 2 else (0,))
            if st == -3:
                # the sigmoid epilogue is promised for C % 16 == 0 only: elsewhere the library may refuse it, with a message, never guess
                assert c.C % 16 != 0 or c.R * c.S > cc.IGEMM_MAX_TAPS, '%s: sigmoid refused on a shape the header promises' % ctx
                assert b'sigmoid' in lib.nnl_last_error(), ctx
                continue
            _compare(mode, y, act_ref(pre_nhwc[has_bias], act), 'y', ctx)
            if stats:
                assert 0 <= bn_rows.value <= rows_max, '%s: bn_rows %d' % (ctx, bn_rows.value)
                if bn_rows.value > 0:
                    pr = part[:bn_rows.value * c.K * 2].view(bn_rows.value, c.K, 2).double()
                    dd = (act_ref(pre_nhwc[has_bias], act) - d['pivot'].view(1, 1, 1, -1)).reshape(-1, c.K).to(DEV)
                    e1 = ((pr[:, :, 0].sum(0) - dd.sum(0)).abs().max() / dd.abs().sum(0).max()).item()
                    e2 = ((pr[:, :, 1].sum(0) - (dd * dd).sum(0)).abs().max() / (dd * dd).sum(0).max()).item()
                    _say('  bn partials: rows %d, relative error of the sums %.2e, of the squares %.2e' % (bn_rows.value, e1, e2))
                    assert e1 < 1e-5 and e2 < 1e-5, '%s: BatchNorm partial sums off by %.2e / %.2e of the largest column' % (ctx, e1, e2)

    # ---- dgrad and wgrad (K % 4 == 0 is part of their contract) ----------------------------------------------------------------
    assert c.K % 4 == 0
    wsb_d = lib.nnl_conv2d_dgrad_workspace_bytes(g)
    for call_mode in CALL_MODES:
        for with_add in (False, True):
            def dgrad(out, ws, wsb, cnt):
                return lib.nnl_conv2d_dgrad(ptr(dy), ptr(wt), ptr(out), g, ptr(add_x) if with_add else None, ptr(ws), wsb, ptr(cnt), stream())
            allowed = not with_add or _addend_allowed(c)
            st, dx, names, ctx = guarded_call('dgrad', 'addend=%d' % with_add, x.numel(), tuple(x.shape), wsb_d, call_mode, dgrad,
                                              accept=(0,) if allowed else (-3,))
            if st == -3:
                assert b'addend' in lib.nnl_last_error(), ctx
                continue
            _compare(mode, dx, dx_ref + d['add_x'].permute(0, 2, 3, 1) if with_add else dx_ref, 'dx', ctx)

    wsb_w = lib.nnl_conv2d_wgrad_workspace_bytes(g)

    def wgrad(out, ws, wsb, cnt):
        return lib.nnl_conv2d_wgrad(ptr(x), ptr(dy), ptr(out), g, ptr(ws), wsb, stream())
    for call_mode in ('ws', 'none'):
        need_ws = call_mode == 'none' and wsb_w > 0
        st, dw, names, ctx = guarded_call('wgrad', 'plain', w.numel(), tuple(w.shape), wsb_w, call_mode, wgrad, accept=(-4,) if need_ws else (0,))
        if st == -4:
            assert b'workspace' in lib.nnl_last_error(), ctx
            continue
        _compare(mode, dw, dw_ref, 'dw', ctx)
    SWEPT.add((cc.case_id(c), mode))


# ---- the census ----------------------------------------------------------------------------------------------------------------------
# Every launch route of the convolution family, read off the dispatcher source (csrc/conv2d.hip: launch_rowk, launch_taps,
# launch_taps_ktail, launch_balanced, nnl_conv2d_dgrad_pre, launch_wgrad_v2, launch_wgrad_wino, launch_wgrad_wino2d, nnl_conv2d_wgrad;
# csrc/wino.hip: nnl_wino_launch; csrc/wino2.hip: nnl_wino2_launch), NOT from a run.  A name is what NNL_ROUTE prints at that site with
# the numeric detail after `@` dropped.  Routes only a switch reaches name the case that sets it (tests/conv_cases.py).
def _bal(bk, extra=('',)):
    return ['balanced<%d>%s%s:%s' % (bk, x, pl, end) for x in extra for pl in (':main_ks', ':tail_slices', ':main_ks:tail_slices')
            for end in ('counters', 'reduce')]


# every name the NNL_ROUTE sites can print (their format strings, all flag combinations): a census name outside this set means a launch
# site was added or renamed without this file being told
KNOWN = set(
    ['rowk<%d,%d>:%s' % (bm, bn, m) for bm, bn in ((64, 64), (128, 64), (64, 128), (128, 128)) for m in ('fwd', 'dgrad')] +
    ['taps<128,128,16>', 'taps<128,128,16>:ncls'] +
    ['taps<64,64,%d>%s%s' % (bk, n, k) for bk in (16, 32) for n in ('', ':ncls') for k in ('', ':ksplit')] +
    ['taps_ktail<16>', 'taps_ktail<32>'] + _bal(16, ('', ':ktail')) + _bal(32, ('', ':ktail')) +
    ['slab_reduce:main', 'slab_reduce:tail', 'dgrad:merged', 'dgrad:per_class', 'dgrad:need_zero'] +
    ['wino1d_filter', 'wino1d_filter:flip', 'wino2d_filter', 'wino2d_filter:flip'] +
    ['wino1d<%d>:%s:%s' % (bk, pl, u) for bk in (16, 32) for pl in ('plain', 'ksliced') for u in ('own_u', 'u_pre')] +
    ['wino2d<%s>:%s:%s' % (t, pl, u) for t in ('32,3', '16,4') for pl in ('plain', 'ksliced') for u in ('own_u', 'u_pre')] +
    ['wino2d<32,4,pos>:own_u', 'wino2d<32,4,pos>:u_pre'] +
    ['wgrad<%s>%s%s' % (t, pr, sp) for t in ('128,128,16,kg1', '128,128,16,kg4', '64,64,32,kg1') for pr in ('', ':pair') for sp in ('', ':splitk')] +
    ['wgrad<%s,kg1>%s' % (t, sp) for t in ('128,64,16', '64,128,16') for sp in ('', ':splitk')] +
    ['wgrad_kmajor<%d,%d>%s' % (bm, bn, sp) for bm, bn in ((64, 64), (128, 64), (64, 128), (128, 128)) for sp in ('', ':splitk')] +
    ['wgrad_wino1d<128,16,kg1>', 'wgrad_wino1d<64,32,kg1>', 'wgrad_wino2d<128,16,kg1>', 'wgrad_wino2d<64,32,kg1>', 'wgrad_wino2d<64,32,kg4>'] +
    ['splitk_reduce', 'wgrad_wino1d_finish', 'wgrad_wino2d_finish'])

# the routes the sweep must reach, per entry point; what KNOWN holds beyond these is accounted for in NOT_REACHED below
ROUTES = {
    'fwd': [
        'rowk<64,64>:fwd', 'rowk<128,64>:fwd', 'rowk<64,128>:fwd', 'rowk<128,128>:fwd',      # bigM-rowk-k36, rowk64x128, bigM-rowk
        'taps<64,64,16>', 'taps<64,64,32>',
        'taps<128,128,16>',                                   # the one-tap Nc >= 8192 rule only (taps128x128-onetap)
        'taps_ktail<16>', 'taps_ktail<32>',
        'balanced<16>:tail_slices:counters', 'balanced<16>:tail_slices:reduce',
        'balanced<32>:tail_slices:counters', 'balanced<32>:tail_slices:reduce',
        'balanced<32>:main_ks:counters', 'balanced<32>:main_ks:reduce',                      # bal-mainks-s2
        'balanced<16>:main_ks:counters', 'balanced<16>:main_ks:reduce',                      # bal16-mainks
        'balanced<16>:main_ks:tail_slices:counters', 'balanced<16>:main_ks:tail_slices:reduce',              # bal16-mainks-tail
        'balanced<32>:ktail:tail_slices:counters', 'balanced<32>:ktail:tail_slices:reduce',  # ktail-bal-tail-fwd
        'balanced<32>:ktail:main_ks:counters', 'balanced<32>:ktail:main_ks:reduce',          # ktail-bal-fwd
        'balanced<16>:ktail:tail_slices:counters', 'balanced<16>:ktail:tail_slices:reduce',  # ktail-bal16
        'balanced<32>:main_ks:tail_slices:counters', 'balanced<32>:main_ks:tail_slices:reduce',
        'slab_reduce:main', 'slab_reduce:tail',
        'wino1d_filter', 'wino1d<16>:plain:own_u', 'wino1d<32>:plain:own_u', 'wino1d<16>:ksliced:own_u', 'wino1d<32>:ksliced:own_u',
        'wino2d_filter', 'wino2d<32,3>:plain:own_u', 'wino2d<16,4>:plain:own_u', 'wino2d<32,3>:ksliced:own_u', 'wino2d<16,4>:ksliced:own_u',
        'wino2d<32,4,pos>:own_u',                             # NNL_WINO2_POS=2: wino2d-pos
    ],
    'dgrad': [
        'rowk<64,64>:dgrad', 'rowk<128,64>:dgrad', 'rowk<64,128>:dgrad', 'rowk<128,128>:dgrad',
        'taps<64,64,16>', 'taps<64,64,32>', 'taps<64,64,16>:ncls', 'taps<64,64,32>:ncls',
        'taps_ktail<16>', 'taps_ktail<32>',
        'dgrad:merged', 'dgrad:per_class', 'dgrad:need_zero',
        'balanced<16>:tail_slices:counters', 'balanced<16>:tail_slices:reduce',
        'balanced<32>:tail_slices:counters', 'balanced<32>:tail_slices:reduce',
        'balanced<32>:main_ks:tail_slices:counters', 'balanced<32>:main_ks:tail_slices:reduce',              # wgrad-wino2d-128 (C = K)
        'balanced<32>:main_ks:counters', 'balanced<32>:main_ks:reduce',                                      # bal32-mainks-dgrad
        'balanced<16>:main_ks:counters', 'balanced<16>:main_ks:reduce',                                      # bal16-mainks-dgrad
        'balanced<16>:main_ks:tail_slices:counters', 'balanced<16>:main_ks:tail_slices:reduce',              # bal16-mainks-tail
        'balanced<32>:ktail:tail_slices:counters', 'balanced<32>:ktail:tail_slices:reduce',                  # ktail-bal-tail
        'balanced<32>:ktail:main_ks:tail_slices:counters', 'balanced<32>:ktail:main_ks:tail_slices:reduce',  # ktail-bal-both
        'balanced<32>:ktail:main_ks:counters', 'balanced<32>:ktail:main_ks:reduce',                          # ktail-bal (K = 1000)
        'slab_reduce:main', 'slab_reduce:tail',
        # the cases with C == K pose the forward's problem again: wino1d-ksliced, wino1d-forced / wino2d-pos without tile counters,
        # wino2d-bk16 (48 channels: the 16-wide k block), wino2d-pos
        # wino2d-ksliced, wino1d-bk16-ksliced
        'wino1d_filter:flip', 'wino1d<32>:ksliced:own_u', 'wino1d<32>:plain:own_u', 'wino1d<16>:ksliced:own_u', 'wino1d<16>:plain:own_u',
        'wino2d_filter:flip', 'wino2d<32,3>:plain:own_u', 'wino2d<16,4>:plain:own_u', 'wino2d<32,3>:ksliced:own_u', 'wino2d<16,4>:ksliced:own_u',
        'wino2d<32,4,pos>:own_u',
    ],
    'wgrad': [
        'wgrad<64,64,32,kg1>', 'wgrad<64,64,32,kg1>:pair', 'wgrad<64,64,32,kg1>:splitk', 'wgrad<64,64,32,kg1>:pair:splitk',
        'wgrad<128,64,16,kg1>:splitk', 'wgrad<64,128,16,kg1>:splitk', 'wgrad<128,128,16,kg4>:pair:splitk',   # wgrad128x64, wgrad64x128, wgrad128x128-kg4
        'splitk_reduce',
        'wgrad_wino1d<64,32,kg1>', 'wgrad_wino1d_finish',     # NNL_WGRAD_WINO=2, NNL_WGRAD_WINO2D=0: wgrad-wino1d
        'wgrad_wino2d<64,32,kg1>', 'wgrad_wino2d<64,32,kg4>', 'wgrad_wino2d<128,16,kg1>', 'wgrad_wino2d_finish',      # kg4: wgrad-wino2d-kg4
        'wgrad_kmajor<64,64>:splitk',                         # N*P*Q >= 2^23: kmajor
    ],
}
assert all(r in KNOWN for rs in ROUTES.values() for r in rs)

# Launch sites the sweep does not reach, and why.  An instantiation that no input can select does not belong here: it is removed from the
# dispatcher, and from KNOWN.
NOT_REACHED = {
    'wgrad<128,128,16,kg1>, wgrad_wino1d<128,16,kg1>':
        'reached only from 1.5e10 flop per pass upwards (64 x 512 x 14 x 14 -> 512 at stride 2; 17 x 128 x 28 x 28 -> 512 under NNL_WGRAD_WINO=2): each '
        'would take the fifth named slot AND 1.5e10 of the 0.3e10 flop the list has left under its 1e11 cap.  The four slots in use go to the 2-D '
        'Winograd-domain kg4 plan (what ResNet-34 takes at 64 images) and the three other direct tile shapes.',
    'balanced<16>:ktail:main_ks*':
        'KTAIL under the 16-wide k block means a (rounded) C below 256, at most 14 k steps per tile; plan_balance needs 8 per slice for '
        'main_ks = 2.  No input selects it.',
    'balanced<32>:ktail:main_ks:tail_slices in the forward':
        'the KTAIL plan with both slicings runs in the dgrad.',
    'the > kTileCounters fallback (more than 65 536 tiles of a sliced plan: second-launch reduce although counters were passed)':
        'needs more than 2^28 output elements, past the size limit of the list.',
    'wino1d / wino2d :u_pre':
        'prepared filters enter through nnl_conv2d_fwd_pre / _dgrad_pre only (tests/test_conv_gpu.py: the prepared-filter window test).',
    'taps<64,64,32>:ksplit': 'nnl_internal_gemm_nt_splitk (the LSTM / linear layers), not a convolution entry point.',
}


def test_every_route_is_reached():
    """the sweep above, in this process, reached every route of ROUTES — and every route met every option of its entry point"""
    assert len(SWEPT) == len(SWEEP), 'the census is filled by test_sweep in the same process: %d of %d sweep items ran' % (len(SWEPT), len(SWEEP))
    table = '\n'.join('%6d  %-6s %s' % (n, e, r) for (e, r), n in sorted(CENSUS.items()))
    _say('census (calls, entry, route):\n' + table)
    missing = [(e, r) for e, rs in ROUTES.items() for r in rs if (e, r) not in CENSUS]
    unknown = [k for k in CENSUS if k[1] not in KNOWN]
    assert not missing and not unknown, 'routes never reached: %s\nroutes no launch site is known to print: %s\ncensus:\n%s' % (missing, unknown, table)
    lacking = []
    for (e, r), labels in sorted(OPTIONS.items()):
        opts = set(o for lab in labels for o in lab.split('|')[0].split(','))
        if e == 'fwd' and not r.startswith(('slab_reduce', 'wino1d_filter', 'wino2d_filter')):
            want = {'bias=0', 'bias=1', 'act=0', 'act=1'}
            if r.startswith(('taps', 'balanced')):
                want |= {'act=2'}                             # the sigmoid epilogue: the tap-table kernels (never a Winograd kernel, refused by row-k)
            if r.startswith(('taps<64,64', 'taps_ktail', 'wino1d<', 'wino2d<')) or (r.startswith('balanced') and r.endswith(':counters')):
                want |= {'stats=1'}                           # the launches that can produce BatchNorm partials
        elif e == 'dgrad' and (r.startswith(('taps<', 'balanced', 'wino1d<', 'wino2d<', 'dgrad:merged')) and 'ktail' not in r):
            want = {'addend=0', 'addend=1'}                   # wherever the header allows an addend: stride 1, and the merged stride-2 launch
        else:
            want = set()
        if not want <= opts:
            lacking.append((e, r, sorted(want - opts)))
    assert not lacking, 'routes that never met an option: %s' % lacking


# ResNet-34 at 64 and 8 images, RetinaNet heads / FPN at 16 images (the geometries CASES of tests/test_conv_gpu.py names), default switches,
# calling mode ws+cnt: the route of each pass, every note of it (the numeric detail after `@` is dropped; the strings with it are printed).
# A planner change shows up as a reviewed diff of this table.
MODEL_SHAPES = [
    (64, 64, 56, 56, 64, 3, 1, 1), (64, 64, 56, 56, 128, 3, 2, 1), (64, 64, 56, 56, 128, 1, 2, 0), (64, 128, 28, 28, 128, 3, 1, 1),
    (64, 256, 14, 14, 256, 3, 1, 1), (64, 512, 7, 7, 512, 3, 1, 1), (64, 4, 224, 224, 64, 7, 2, 3),
    (8, 64, 56, 56, 64, 3, 1, 1), (8, 128, 28, 28, 128, 3, 1, 1), (8, 256, 14, 14, 256, 3, 1, 1), (8, 512, 7, 7, 512, 3, 1, 1),
    (16, 256, 64, 64, 256, 3, 1, 1), (16, 256, 32, 32, 256, 3, 1, 1), (16, 256, 16, 16, 256, 3, 1, 1), (16, 256, 8, 8, 256, 3, 1, 1),
    (16, 256, 4, 4, 256, 3, 1, 1), (16, 256, 16, 16, 36, 3, 1, 1), (16, 256, 8, 8, 180, 3, 1, 1), (16, 512, 16, 16, 256, 1, 1, 0),
    (16, 256, 16, 16, 256, 3, 2, 1),
]
MODEL_ROUTES = {
    (64, 64, 56, 56, 64, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<16,4>:ksliced:own_u',
    (64, 64, 56, 56, 64, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<16,4>:ksliced:own_u',
    (64, 64, 56, 56, 64, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg4>;wgrad_wino2d_finish',
    (64, 64, 56, 56, 128, 3, 2, 1, 'fwd'): 'balanced<32>:tail_slices:counters',
    (64, 64, 56, 56, 128, 3, 2, 1, 'dgrad'): 'dgrad:merged;taps<64,64,16>:ncls',
    (64, 64, 56, 56, 128, 3, 2, 1, 'wgrad'): 'wgrad<64,64,32,kg1>:pair:splitk;splitk_reduce',
    (64, 64, 56, 56, 128, 1, 2, 0, 'fwd'): 'taps<64,64,32>',
    (64, 64, 56, 56, 128, 1, 2, 0, 'dgrad'): 'dgrad:need_zero;dgrad:per_class;taps<64,64,32>',
    (64, 64, 56, 56, 128, 1, 2, 0, 'wgrad'): 'wgrad<64,64,32,kg1>:pair:splitk;splitk_reduce',
    (64, 128, 28, 28, 128, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,3>:ksliced:own_u',
    (64, 128, 28, 28, 128, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,3>:ksliced:own_u',
    (64, 128, 28, 28, 128, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg4>;wgrad_wino2d_finish',
    (64, 256, 14, 14, 256, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,4,pos>:own_u',
    (64, 256, 14, 14, 256, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,4,pos>:own_u',
    (64, 256, 14, 14, 256, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg4>;wgrad_wino2d_finish',
    (64, 512, 7, 7, 512, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,4,pos>:own_u',
    (64, 512, 7, 7, 512, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,4,pos>:own_u',
    (64, 512, 7, 7, 512, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<128,16,kg1>;wgrad_wino2d_finish',
    (64, 4, 224, 224, 64, 7, 2, 3, 'fwd'): 'rowk<128,64>:fwd',
    (64, 4, 224, 224, 64, 7, 2, 3, 'dgrad'): 'dgrad:merged;taps<64,64,32>:ncls',
    (64, 4, 224, 224, 64, 7, 2, 3, 'wgrad'): 'wgrad<64,128,16,kg1>:splitk;splitk_reduce',
    (8, 64, 56, 56, 64, 3, 1, 1, 'fwd'): 'wino1d_filter;wino1d<32>:plain:own_u',
    (8, 64, 56, 56, 64, 3, 1, 1, 'dgrad'): 'wino1d_filter:flip;wino1d<32>:plain:own_u',
    (8, 64, 56, 56, 64, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg1>;wgrad_wino2d_finish',
    (8, 128, 28, 28, 128, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,4,pos>:own_u',
    (8, 128, 28, 28, 128, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,4,pos>:own_u',
    (8, 128, 28, 28, 128, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg1>;wgrad_wino2d_finish',
    (8, 256, 14, 14, 256, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,4,pos>:own_u',
    (8, 256, 14, 14, 256, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,4,pos>:own_u',
    (8, 256, 14, 14, 256, 3, 1, 1, 'wgrad'): 'wgrad<64,64,32,kg1>:pair:splitk;splitk_reduce',
    (8, 512, 7, 7, 512, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,4,pos>:own_u',
    (8, 512, 7, 7, 512, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,4,pos>:own_u',
    (8, 512, 7, 7, 512, 3, 1, 1, 'wgrad'): 'wgrad<64,64,32,kg1>:pair',
    (16, 256, 64, 64, 256, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<16,4>:plain:own_u',
    (16, 256, 64, 64, 256, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<16,4>:plain:own_u',
    (16, 256, 64, 64, 256, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<128,16,kg1>;wgrad_wino2d_finish',
    (16, 256, 32, 32, 256, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,4,pos>:own_u',
    (16, 256, 32, 32, 256, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,4,pos>:own_u',
    (16, 256, 32, 32, 256, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg4>;wgrad_wino2d_finish',
    (16, 256, 16, 16, 256, 3, 1, 1, 'fwd'): 'wino2d_filter;wino2d<32,4,pos>:own_u',
    (16, 256, 16, 16, 256, 3, 1, 1, 'dgrad'): 'wino2d_filter:flip;wino2d<32,4,pos>:own_u',
    (16, 256, 16, 16, 256, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg1>;wgrad_wino2d_finish',
    (16, 256, 8, 8, 256, 3, 1, 1, 'fwd'): 'balanced<32>:main_ks:counters',
    (16, 256, 8, 8, 256, 3, 1, 1, 'dgrad'): 'balanced<32>:main_ks:counters',
    (16, 256, 8, 8, 256, 3, 1, 1, 'wgrad'): 'wgrad<64,64,32,kg1>:pair:splitk;splitk_reduce',
    (16, 256, 4, 4, 256, 3, 1, 1, 'fwd'): 'balanced<32>:tail_slices:counters',
    (16, 256, 4, 4, 256, 3, 1, 1, 'dgrad'): 'balanced<32>:tail_slices:counters',
    (16, 256, 4, 4, 256, 3, 1, 1, 'wgrad'): 'wgrad<64,64,32,kg1>:pair',
    (16, 256, 16, 16, 36, 3, 1, 1, 'fwd'): 'balanced<32>:main_ks:counters',
    (16, 256, 16, 16, 36, 3, 1, 1, 'dgrad'): 'rowk<64,64>:dgrad',
    (16, 256, 16, 16, 36, 3, 1, 1, 'wgrad'): 'wgrad_wino2d<64,32,kg1>;wgrad_wino2d_finish',
    (16, 256, 8, 8, 180, 3, 1, 1, 'fwd'): 'balanced<32>:tail_slices:counters',
    (16, 256, 8, 8, 180, 3, 1, 1, 'dgrad'): 'rowk<64,64>:dgrad',
    (16, 256, 8, 8, 180, 3, 1, 1, 'wgrad'): 'wgrad<64,64,32,kg1>:pair:splitk;splitk_reduce',
    (16, 512, 16, 16, 256, 1, 1, 0, 'fwd'): 'taps<64,64,32>',
    (16, 512, 16, 16, 256, 1, 1, 0, 'dgrad'): 'taps<64,64,32>',
    (16, 512, 16, 16, 256, 1, 1, 0, 'wgrad'): 'wgrad<64,64,32,kg1>:pair:splitk;splitk_reduce',
    (16, 256, 16, 16, 256, 3, 2, 1, 'fwd'): 'balanced<32>:main_ks:counters',
    (16, 256, 16, 16, 256, 3, 2, 1, 'dgrad'): 'dgrad:merged;taps<64,64,32>:ncls',
    (16, 256, 16, 16, 256, 3, 2, 1, 'wgrad'): 'wgrad<64,64,32,kg1>:pair:splitk;splitk_reduce',
}


def test_default_routes_of_the_model_shapes():
    from neuralnetworklibrary_amd import _lib, ops
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    lib.nnl_reload_env()
    got, full = {}, {}
    for (N, C, H, W, K, R, stride, pad) in MODEL_SHAPES:
        P, Q = cc.out_size(H, R, stride, pad), cc.out_size(W, R, stride, pad)
        geom = _lib.ConvGeom(N, H, W, C, K, R, R, stride, pad, P, Q)
        g = ctypes.byref(geom)
        x, w, y = torch.zeros(N, H, W, C, device=DEV), torch.zeros(K, R, R, C, device=DEV), torch.zeros(N, P, Q, K, device=DEV)
        cnt = ops._tile_counters(x.device)
        key = (N, C, H, W, K, R, stride, pad)

        def ws_of(nbytes):
            return torch.empty(nbytes // 4 + 4, device=DEV), nbytes
        ws, wsb = ws_of(lib.nnl_conv2d_fwd_workspace_bytes(g))
        st, names, _ = _routes_of(lib, lambda: lib.nnl_conv2d_fwd(ptr(x), ptr(w), None, ptr(y), g, 0, ptr(ws), wsb, ptr(cnt), None, None, None, stream()))
        assert st == 0
        got[key + ('fwd',)], full[key + ('fwd',)] = ';'.join(n.split('@')[0] for n in names), ';'.join(names)
        if K % 4 == 0:
            ws, wsb = ws_of(lib.nnl_conv2d_dgrad_workspace_bytes(g))
            wt = torch.zeros(C, R, R, K, device=DEV)
            st, names, _ = _routes_of(lib, lambda: lib.nnl_conv2d_dgrad(ptr(y), ptr(wt), ptr(x), g, None, ptr(ws), wsb, ptr(cnt), stream()))
            assert st == 0
            got[key + ('dgrad',)], full[key + ('dgrad',)] = ';'.join(n.split('@')[0] for n in names), ';'.join(names)
            ws, wsb = ws_of(lib.nnl_conv2d_wgrad_workspace_bytes(g))
            st, names, _ = _routes_of(lib, lambda: lib.nnl_conv2d_wgrad(ptr(x), ptr(y), ptr(w), g, ptr(ws), wsb, stream()))
            assert st == 0
            got[key + ('wgrad',)], full[key + ('wgrad',)] = ';'.join(n.split('@')[0] for n in names), ';'.join(names)
        torch.cuda.synchronize()
    table = '\n'.join('    %r: %r,' % kv for kv in got.items())
    _say('routes of the model shapes:\n' + '\n'.join('    %r: %r' % kv for kv in full.items()))
    assert got == MODEL_ROUTES, 'the default routes of the model shapes changed; the table now reads\n' + table
