"""The BatchNorm C ABI (nnl_bn_fwd / nnl_bn_bwd, the nnl_bn_sync_* entries, nnl_bn_relu_maxpool_*; include/nnl.h) called directly over the
launch regimes of csrc/batchnorm.hip, against the fp64 reference of tests/bn_cases.py.

Every case of bn_cases.CASES runs in three data modes (`int`: exact sums, see bn_cases; `randn` and `randn+40`: the project's
tolerances, mean offset 0 and 40) and in every calling mode of CONFIGS: training / eval, residual or not, ReLU with the keep-bit mask /
ReLU with y and relu_mask = NULL / no ReLU, dres, dgamma and dbeta NULL or not, gamma and beta NULL, running statistics and
num_batches_tracked NULL in training.

Around every call: outputs, mask and workspace sit inside larger allocations with sentinel bands, outputs are pre-filled with NaN, the
mask has exactly the documented ceil(rows*C/32) + 2 words, and the call is repeated and must reproduce itself bit for bit.

The backward reference takes its ReLU gate from the kernel's own forward output, which the forward check has tied to fp64 before: a
value that rounds across zero cannot move dx by O(1) then.

The file takes about 15 s on an MI355X (the largest case 1.3 s), a twentieth of the rest of the GPU suite.
"""
import ctypes
import sys

import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                                     # elements of sentinel on either side of a buffer
SENT = {torch.float32: 12345.0, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A, torch.uint8: 0xA5}
MODES = [('int', 0.0), ('randn', 0.0), ('randn+40', 40.0)]

CONFIGS = [   # relu: 'mask' (keep bits to the backward), 'y' (relu_mask NULL in both calls, the backward gates from y), None
    dict(name='train+res+relu(mask)', training=1, res=1, relu='mask', affine=1, running=1, nbt=1, dres=1, dgb=1, pivot=1),
    dict(name='train,relu(y),plain', training=1, res=0, relu='y', affine=0, running=0, nbt=0, dres=0, dgb=0, pivot=0),
    dict(name='train+res,linear', training=1, res=1, relu=None, affine=1, running=1, nbt=0, dres=1, dgb=1, pivot=0),
    dict(name='eval+res+relu(mask)', training=0, res=1, relu='mask', affine=1, running=1, nbt=1, dres=1, dgb=1, pivot=0),
    dict(name='eval,relu(y),plain', training=0, res=0, relu='y', affine=0, running=1, nbt=0, dres=0, dgb=0, pivot=0),
]


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


class Guarded:
    """`numel` elements inside a larger allocation with sentinel bands on both sides"""

    def __init__(self, numel, fill, dtype=torch.float32):
        self.numel, self.sent = numel, SENT[dtype]
        self.buf = torch.full((numel + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + numel]
        if torch.is_tensor(fill):
            self.t.copy_(fill.reshape(-1))
        else:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[GUARD + self.numel:] == self.sent).all())


def _nan(numel):
    return Guarded(numel, float('nan'))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _check_bands(bufs, ctx):
    for name, g in bufs.items():
        if g is not None:
            assert g.intact(), '%s: wrote outside %s (guard band touched)' % (ctx, name)


def _written(t, what, ctx):
    assert not bool(torch.isnan(t).any()), '%s: %d elements of %s were never written (NaN sentinel)' % (ctx, int(torch.isnan(t).sum()), what)


def _close(got, ref64, tol, what, ctx, atol_rel=False, atol_add=0.0):
    """|got - ref| <= atol + rtol*|ref|, compared on the device; atol_rel: atol = tol[1] * max|ref| (+ atol_add)"""
    _written(got, what, ctx)
    ref = ref64.to(DEV)
    rtol, atol = tol
    if atol_rel:
        atol = atol * float(ref.abs().max()) + atol_add
    err = (got.double() - ref).abs()
    lim = atol + rtol * ref.abs()
    if not bool((err <= lim).all()):
        i = tuple(int(v) for v in torch.unravel_index((err - lim).argmax(), err.shape))
        raise AssertionError('%s: %s max abs err %.3e, worst at %s: got %r, want %r, tolerance there %.3e' %
                             (ctx, what, err.max().item(), i, got[i].item(), ref[i].item(), lim[i].item()))


def _keep_bits(mask, numel):
    """bit e of the flat element index, as bool [numel]"""
    sh = torch.arange(32, device=DEV, dtype=torch.int32)
    return ((mask.view(-1, 1) >> sh) & 1).view(-1)[:numel].bool()


def _mask_words(rows, C):
    return (rows * C + 31) // 32 + 2


def _workspace(lib, rows, C):
    wsb = int(lib.nnl_bn_workspace_bytes(rows, C))
    assert wsb % 4 == 0 and wsb > 0
    return _nan(wsb // 4), wsb


def _twice(run, ctx):
    a = run()
    b = run()
    assert _same(a, b), '%s: two runs differ (not bitwise reproducible)' % ctx
    return a


# ---- nnl_bn_fwd / nnl_bn_bwd over the launch regimes ---------------------------------------------------------------------------------------------
SWEEP = [(c, m) for m in MODES for c in bc.CASES]


@pytest.mark.parametrize('case,mode', SWEEP, ids=['%s-%s' % (bc.case_id(c), m[0]) for c, m in SWEEP])
def test_sweep(case, mode):
    """The randn+40 mode found that y = x*scale + shift loses 2^-23 * |mean*scale| (1x4 training, n = 1: 4.3e-4 against a tolerance of
    2.8e-5; 9000x513 eval: 1.06e-5 against 1.006e-5); nnl_bn_fwd now centres the channels whose |mean*scale| exceeds 16 (include/nnl.h)."""
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    rows, C = case.rows, case.C
    mname, offset = mode
    is_int = mname == 'int'
    d = bc.make_data(rows, C, 'int' if is_int else 'randn', offset, seed=bc.CASES.index(case))
    x64, dy64, res64 = d['x'].double(), d['dy'].double(), d['res'].double()
    n = float(rows)
    bmean, bvar = bc.batch_stats(x64)
    if is_int:
        S1, S2 = bc.shifted_sums(x64, x64[0])
        exact = bc.stats_from_sums(S1, S2, x64[0], n, d['rmean'].double(), d['rvar'].double())
    x, dy, res = d['x'].to(DEV), d['dy'].to(DEV), d['res'].to(DEV)
    nel = rows * C

    for cfg in CONFIGS:
        ctx = '%s [%s] %s' % (bc.case_id(case), mname, cfg['name'])
        _say('case', ctx)
        training, relu = cfg['training'], cfg['relu']
        gamma = d['gamma'].to(DEV) if cfg['affine'] else None
        beta = d['beta'].to(DEV) if cfg['affine'] else None
        g64 = d['gamma'].double() if cfg['affine'] else None
        b64 = d['beta'].double() if cfg['affine'] else None
        r64 = res64 if cfg['res'] else None
        nbt0 = 41

        def forward():
            o = dict(y=_nan(nel), mean=_nan(C), invstd=_nan(C),
                     rmean=Guarded(C, d['rmean']) if cfg['running'] else None, rvar=Guarded(C, d['rvar']) if cfg['running'] else None,
                     nbt=Guarded(1, nbt0, torch.int64) if cfg['nbt'] else None,
                     mask=Guarded(_mask_words(rows, C), 0x33333333, torch.int32) if relu == 'mask' else None,
                     pivot=_nan(C) if cfg['pivot'] else None)
            ws, wsb = _workspace(lib, rows, C)
            o['workspace'] = ws
            p = lambda k: ptr(o[k].t) if o[k] is not None else None
            st = lib.nnl_bn_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(res) if cfg['res'] else None, p('y'), p('mean'), p('invstd'), p('rmean'),
                                p('rvar'), rows, C, bc.EPS, bc.MOMENTUM, training, 1 if relu else 0, p('nbt'), p('mask'), None, 0, None,
                                p('pivot'), ptr(ws.t), wsb, stream())
            torch.cuda.synchronize()
            assert st == 0, '%s: nnl_bn_fwd status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
            _check_bands(o, ctx + ' fwd')
            return {k: (v.t if v is not None else None) for k, v in o.items() if k != 'workspace'}

        f = _twice(forward, ctx + ' fwd')
        y = f['y'].view(rows, C)
        _written(y, 'y', ctx)

        # ---- statistics ---------------------------------------------------------------------------------------------------------
        if training:
            mean64, var64 = bmean, bvar
            if is_int:
                for k, got in (('mean', f['mean']), ('invstd', f['invstd'])) + ((('rmean', f['rmean']), ('rvar', f['rvar'])) if cfg['running'] else ()):
                    _written(got, k, ctx)
                    # bound: the count of fp32 roundings in the header's expression, derived in bn_cases.stats_from_sums
                    assert bc.within(got.cpu(), exact[k], exact[k + '_bound']), '%s: %s outside its rounding bound: %s' % (
                        ctx, k, bc.worst(got.cpu(), exact[k], exact[k + '_bound']))
            else:
                _close(f['mean'], mean64, bc.TOL_RMEAN, 'save_mean', ctx)
                _close(f['invstd'], 1.0 / torch.sqrt(var64 + bc.EPS32), bc.TOL_RVAR, 'save_invstd', ctx)
                if cfg['running']:
                    _close(f['rmean'], bc.running_update(d['rmean'].double(), mean64, bc.MOM32), bc.TOL_RMEAN, 'running_mean', ctx)
                    _close(f['rvar'], bc.running_update(d['rvar'].double(), bc.unbiased(var64, n), bc.MOM32), bc.TOL_RVAR, 'running_var', ctx)
            if cfg['nbt']:
                assert int(f['nbt']) == nbt0 + 1, '%s: num_batches_tracked %d' % (ctx, int(f['nbt']))
            if cfg['pivot']:
                assert torch.equal(_bits(f['pivot']), _bits(f['mean'])), '%s: pivot_out != save_mean' % ctx
        else:
            mean64, var64 = d['rmean'].double(), d['rvar'].double()
            assert torch.equal(f['rmean'].cpu(), d['rmean']) and torch.equal(f['rvar'].cpu(), d['rvar']), '%s: eval changed the running statistics' % ctx
            assert torch.equal(f['mean'].cpu(), d['rmean']), '%s: eval save_mean != running_mean' % ctx
            # t = fl(rv + eps), sqrt, 1/s: relative error <= U/2 + U + U
            want = 1.0 / torch.sqrt(var64 + bc.EPS32)
            assert bc.within(f['invstd'].cpu(), want, 2.5 * 1.01 * bc.U * want), '%s: eval save_invstd: %s' % (
                ctx, bc.worst(f['invstd'].cpu(), want, 2.5 * 1.01 * bc.U * want))
            if cfg['nbt']:
                assert int(f['nbt']) == nbt0, '%s: eval incremented num_batches_tracked' % ctx

        # ---- y and the keep bits --------------------------------------------------------------------------------------------------
        yref, invstd64 = bc.bn_fwd_ref(x64, g64, b64, r64, mean64, var64, bc.EPS32, bool(relu))
        _close(y, yref, bc.TOL_Y, 'y', ctx)
        keep = y > 0
        if relu == 'mask':
            got = _keep_bits(f['mask'], nel).view(rows, C)
            assert torch.equal(got, keep), '%s: %d keep bits differ from y > 0 of the kernel\'s own y' % (ctx, int((got != keep).sum()))

        # ---- backward ---------------------------------------------------------------------------------------------------------------
        def backward():
            o = dict(dx=_nan(nel), dres=_nan(nel) if cfg['dres'] else None, dgamma=_nan(C) if cfg['dgb'] else None,
                     dbeta=_nan(C) if cfg['dgb'] else None)
            ws, wsb = _workspace(lib, rows, C)
            o['workspace'] = ws
            p = lambda k: ptr(o[k].t) if o[k] is not None else None
            st = lib.nnl_bn_bwd(ptr(dy), ptr(y) if relu == 'y' else None, ptr(f['mask']) if relu == 'mask' else None, ptr(x), ptr(gamma),
                                ptr(f['mean']), ptr(f['invstd']), p('dx'), p('dres'), p('dgamma'), p('dbeta'), rows, C, training,
                                1 if relu else 0, ptr(ws.t), wsb, stream())
            torch.cuda.synchronize()
            assert st == 0, '%s: nnl_bn_bwd status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
            _check_bands(o, ctx + ' bwd')
            return {k: (v.t if v is not None else None) for k, v in o.items() if k != 'workspace'}

        b = _twice(backward, ctx + ' bwd')
        gate = keep.cpu().double() if relu else None
        ref = bc.bn_bwd_ref(dy64, gate, x64, g64, mean64, invstd64, bool(training))
        if cfg['dres']:
            _written(b['dres'], 'dres', ctx)
            assert torch.equal(b['dres'].view(rows, C), torch.where(keep, dy, torch.zeros_like(dy)) if relu else dy), '%s: dres is not the gated dy, bit for bit' % ctx
        if cfg['dgb']:
            if is_int:
                _written(b['dbeta'], 'dbeta', ctx)
                assert torch.equal(b['dbeta'].cpu().double(), ref['dbeta']), '%s: dbeta differs from the exact sum in %d channels, e.g. %s' % (
                    ctx, int((b['dbeta'].cpu().double() != ref['dbeta']).sum()), bc.worst(b['dbeta'].cpu(), ref['dbeta'], torch.zeros(C, dtype=torch.float64)))
            else:
                _close(b['dbeta'], ref['dbeta'], bc.TOL_DPARAM, 'dbeta', ctx, atol_rel=True)
            _close(b['dgamma'], ref['dgamma'], bc.TOL_DPARAM, 'dgamma', ctx, atol_rel=True)
        _close(b['dx'].view(rows, C), ref['dx'], bc.TOL_DX, 'dx', ctx, atol_rel=True, atol_add=1e-7)


def test_refusals_before_any_launch():
    """arguments the entry points check on the host: nothing is launched"""
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    t = torch.zeros(64, device=DEV)
    ws, wsb = _workspace(lib, 4, 4)
    args = lambda rows, C, training, wsb_: (ptr(t), None, None, None, ptr(t), ptr(t), ptr(t), None, None, rows, C, bc.EPS, bc.MOMENTUM, training, 0,
                                            None, None, None, 0, None, None, ptr(ws.t), wsb_, stream())
    assert lib.nnl_bn_fwd(*args(0, 4, 1, wsb)) == -1 and b'bad sizes' in lib.nnl_last_error()
    assert lib.nnl_bn_fwd(*args(4, 4, 0, wsb)) == -1 and b'eval mode needs running statistics' in lib.nnl_last_error()
    assert lib.nnl_bn_fwd(*args(4, 4, 1, wsb - 4)) != 0 and b'workspace too small' in lib.nnl_last_error()
    st = lib.nnl_bn_bwd(ptr(t), None, None, ptr(t), None, ptr(t), ptr(t), ptr(t), None, None, None, 4, 4, 1, 1, ptr(ws.t), wsb, stream())
    assert st == -1 and b'null pointer' in lib.nnl_last_error()            # ReLU without y and without mask
    torch.cuda.synchronize()
    assert ws.intact() and bool(torch.isnan(ws.t).all()) and float(t.abs().sum()) == 0


# ---- statistics from conv-epilogue partials: both finalize widths ------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('tiles,C', bc.EXT_CASES, ids=['%dx%d' % tc for tc in bc.EXT_CASES])
def test_ext_partials(tiles, C, mode):
    """nnl_bn_fwd with ext_partials: the statistics come from per-tile shifted sums (laid out [tile][C][2]) around a given pivot, synthesised
    on the host — no convolution.  The reference evaluates the same fp32 partials in fp64."""
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    mname, offset = mode
    is_int = mname == 'int'
    rows = bc.ext_rows_of(tiles)
    d = bc.make_data(rows, C, 'int' if is_int else 'randn', offset, seed=tiles)
    x64 = d['x'].double()
    g = torch.Generator().manual_seed(tiles + C)
    pivot = torch.randint(-4, 5, (C,), generator=g).float() if is_int else (x64.mean(0) + 0.1 * torch.randn(C, generator=g).double()).float()
    dd = torch.zeros(tiles * bc.EXT_TILE, C, dtype=torch.float64)
    dd[:rows] = x64 - pivot.double()
    dd = dd.view(tiles, bc.EXT_TILE, C)
    part = torch.stack([dd.sum(1), (dd * dd).sum(1)], dim=2).float()                  # [tile][C][2]
    p64 = part.double()
    if is_int:
        assert torch.equal(p64[..., 0], dd.sum(1)) and torch.equal(p64[..., 1], (dd * dd).sum(1))
    S1, S2 = p64[..., 0].sum(0), p64[..., 1].sum(0)
    n = float(rows)
    exact = bc.stats_from_sums(S1, S2, pivot.double(), n, d['rmean'].double(), d['rvar'].double())
    ctx = 'ext %d tiles x %d [%s]' % (tiles, C, mname)
    x, part_d, pivot_d = d['x'].to(DEV), part.to(DEV), Guarded(C, pivot)
    gamma, beta = d['gamma'].to(DEV), d['beta'].to(DEV)
    nel = rows * C

    def forward():
        o = dict(y=_nan(nel), mean=_nan(C), invstd=_nan(C), rmean=Guarded(C, d['rmean']), rvar=Guarded(C, d['rvar']),
                 nbt=Guarded(1, 7, torch.int64), pivot_out=_nan(C), ext_pivot=pivot_d)
        ws, wsb = _workspace(lib, rows, C)
        o['workspace'] = ws
        p = lambda k: ptr(o[k].t)
        st = lib.nnl_bn_fwd(ptr(x), ptr(gamma), ptr(beta), None, p('y'), p('mean'), p('invstd'), p('rmean'), p('rvar'), rows, C, bc.EPS,
                            bc.MOMENTUM, 1, 0, p('nbt'), None, ptr(part_d), tiles, p('ext_pivot'), p('pivot_out'), ptr(ws.t), wsb, stream())
        torch.cuda.synchronize()
        assert st == 0, '%s: status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
        _check_bands(o, ctx)
        return {k: v.t for k, v in o.items() if k != 'workspace'}

    f = _twice(forward, ctx)
    assert torch.equal(f['ext_pivot'].cpu(), pivot), '%s: ext_pivot was written' % ctx
    assert int(f['nbt']) == 8 and torch.equal(_bits(f['pivot_out']), _bits(f['mean']))
    if is_int:
        for k in ('mean', 'invstd', 'rmean', 'rvar'):
            assert bc.within(f[k].cpu(), exact[k], exact[k + '_bound']), '%s: %s outside its rounding bound: %s' % (
                ctx, k, bc.worst(f[k].cpu(), exact[k], exact[k + '_bound']))
    else:
        _close(f['mean'], exact['mean'], bc.TOL_RMEAN, 'save_mean', ctx)
        _close(f['invstd'], exact['invstd'], bc.TOL_RVAR, 'save_invstd', ctx)
        _close(f['rmean'], exact['rmean'], bc.TOL_RMEAN, 'running_mean', ctx)
        _close(f['rvar'], exact['rvar'], bc.TOL_RVAR, 'running_var', ctx)
    yref, _ = bc.bn_fwd_ref(x64, d['gamma'].double(), d['beta'].double(), None, exact['mean'], exact['var'], bc.EPS32, False)
    _close(f['y'].view(rows, C), yref, bc.TOL_Y, 'y', ctx)


# ---- the split-phase cross-replica entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('C,split', bc.SYNC_CASES, ids=['%dx%s' % (C, '+'.join(map(str, s))) for C, s in bc.SYNC_CASES])
def test_sync_entries(C, split, mode):
    """nnl_bn_sync_stats -> (the host stacks the ranks' real stats in place of the all_gather) -> nnl_bn_sync_fwd; nnl_bn_sync_bwd_reduce ->
    (the host adds the ranks' sums in rank order in place of the all_reduce) -> nnl_bn_sync_bwd.  Mean, variance and dx must be the
    whole-batch fp64 values, the running statistics bit-identical on every rank."""
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    mname, offset = mode
    is_int = mname == 'int'
    world, total = len(split), sum(split)
    d = bc.make_data(total, C, 'int' if is_int else 'randn', offset, seed=world)
    x64, dy64, res64 = d['x'].double(), d['dy'].double(), d['res'].double()
    mean64, var64 = bc.batch_stats(x64)
    lo = [sum(split[:r]) for r in range(world)]
    xs = [d['x'][lo[r]:lo[r] + split[r]].contiguous().to(DEV) for r in range(world)]
    dys = [d['dy'][lo[r]:lo[r] + split[r]].contiguous().to(DEV) for r in range(world)]
    ress = [d['res'][lo[r]:lo[r] + split[r]].contiguous().to(DEV) for r in range(world)]
    gamma, beta = d['gamma'].to(DEV), d['beta'].to(DEV)
    ctx0 = 'sync C=%d split=%s [%s]' % (C, split, mname)

    all_stats = torch.empty(world, 2 * C + 2, device=DEV)
    for r in range(world):
        ctx = '%s rank %d stats' % (ctx0, r)

        def stats():
            o = dict(stats=_nan(2 * C + 2))
            ws, wsb = _workspace(lib, split[r], C)
            o['workspace'] = ws
            st = lib.nnl_bn_sync_stats(ptr(xs[r]), ptr(o['stats'].t), split[r], C, ptr(ws.t), wsb, stream())
            torch.cuda.synchronize()
            assert st == 0, '%s: status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
            _check_bands(o, ctx)
            return dict(stats=o['stats'].t)

        s = _twice(stats, ctx)['stats']
        _written(s, 'stats', ctx)
        m_r, M2_r, hi, low = bc.sync_local_ref(x64[lo[r]:lo[r] + split[r]])
        assert s[2 * C].item() == hi and s[2 * C + 1].item() == low, '%s: row count travels as %r * 65536 + %r' % (ctx, s[2 * C].item(), s[2 * C + 1].item())
        _close(s[:C], m_r, bc.TOL_RMEAN, 'local mean', ctx)
        _close(s[C:2 * C], M2_r, bc.TOL_RVAR, 'local M2', ctx, atol_rel=True)
        all_stats[r] = s
    assert max(split) < 65536 or float(all_stats[:, 2 * C].max()) >= 1.0

    yref, invstd64 = bc.bn_fwd_ref(x64, d['gamma'].double(), d['beta'].double(), res64, mean64, var64, bc.EPS32, True)
    fw = []
    for r in range(world):
        ctx = '%s rank %d fwd' % (ctx0, r)
        nel = split[r] * C

        def forward():
            o = dict(y=_nan(nel), mean=_nan(C), invstd=_nan(C), rmean=Guarded(C, d['rmean']), rvar=Guarded(C, d['rvar']),
                     nbt=Guarded(1, 3, torch.int64), mask=Guarded(_mask_words(split[r], C), 0x33333333, torch.int32))
            ws, wsb = _workspace(lib, split[r], C)
            o['workspace'] = ws
            p = lambda k: ptr(o[k].t)
            st = lib.nnl_bn_sync_fwd(ptr(xs[r]), ptr(all_stats), world, ptr(gamma), ptr(beta), ptr(ress[r]), p('y'), p('mean'), p('invstd'),
                                     p('rmean'), p('rvar'), split[r], C, bc.EPS, bc.MOMENTUM, 1, p('nbt'), p('mask'), ptr(ws.t), wsb, stream())
            torch.cuda.synchronize()
            assert st == 0, '%s: status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
            _check_bands(o, ctx)
            return {k: v.t for k, v in o.items() if k != 'workspace'}

        f = _twice(forward, ctx)
        fw.append(f)
        _close(f['mean'], mean64, bc.TOL_RMEAN, 'mean', ctx)
        _close(f['invstd'], invstd64, bc.TOL_RVAR, 'invstd', ctx)
        _close(f['rmean'], bc.running_update(d['rmean'].double(), mean64, bc.MOM32), bc.TOL_RMEAN, 'running_mean', ctx)
        _close(f['rvar'], bc.running_update(d['rvar'].double(), bc.unbiased(var64, float(total)), bc.MOM32), bc.TOL_RVAR, 'running_var', ctx)
        assert int(f['nbt']) == 4
        y = f['y'].view(split[r], C)
        _close(y, yref[lo[r]:lo[r] + split[r]], bc.TOL_Y, 'y', ctx)
        assert torch.equal(_keep_bits(f['mask'], nel).view(split[r], C), y > 0), '%s: keep bits differ from y > 0' % ctx
        for k in ('mean', 'invstd', 'rmean', 'rvar'):
            assert torch.equal(_bits(f[k]), _bits(fw[0][k])), '%s: %s differs from rank 0 (not bit-identical across ranks)' % (ctx, k)

    gate64 = torch.cat([(fw[r]['y'].view(split[r], C) > 0).cpu() for r in range(world)]).double()
    whole = bc.bn_bwd_ref(dy64, gate64, x64, d['gamma'].double(), mean64, invstd64, True)
    sums = []
    for r in range(world):
        ctx = '%s rank %d bwd_reduce' % (ctx0, r)

        def reduce():
            o = dict(sums=_nan(2 * C))
            ws, wsb = _workspace(lib, split[r], C)
            o['workspace'] = ws
            st = lib.nnl_bn_sync_bwd_reduce(ptr(dys[r]), None, ptr(fw[r]['mask']), ptr(xs[r]), ptr(fw[r]['mean']), ptr(fw[r]['invstd']),
                                            ptr(o['sums'].t), split[r], C, 1, ptr(ws.t), wsb, stream())
            torch.cuda.synchronize()
            assert st == 0, '%s: status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
            _check_bands(o, ctx)
            return dict(sums=o['sums'].t)

        sums.append(_twice(reduce, ctx)['sums'])
    total_sums = sums[0].clone()
    for r in range(1, world):
        total_sums += sums[r]

    for r in range(world):
        ctx = '%s rank %d bwd' % (ctx0, r)
        nel = split[r] * C
        sl = slice(lo[r], lo[r] + split[r])
        local = bc.bn_bwd_ref(dy64[sl], gate64[sl], x64[sl], d['gamma'].double(), mean64, invstd64, True, n=float(total),
                              sums=(whole['dbeta'], whole['dgamma']))

        def backward():
            o = dict(dx=_nan(nel), dres=_nan(nel), dgamma=_nan(C), dbeta=_nan(C))
            ws, wsb = _workspace(lib, split[r], C)
            o['workspace'] = ws
            p = lambda k: ptr(o[k].t)
            st = lib.nnl_bn_sync_bwd(ptr(dys[r]), None, ptr(fw[r]['mask']), ptr(xs[r]), ptr(gamma), ptr(fw[r]['mean']), ptr(fw[r]['invstd']),
                                     ptr(sums[r]), ptr(total_sums), ptr(all_stats), world, p('dx'), p('dres'), p('dgamma'), p('dbeta'),
                                     split[r], C, 1, ptr(ws.t), wsb, stream())
            torch.cuda.synchronize()
            assert st == 0, '%s: status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
            _check_bands(o, ctx)
            return {k: v.t for k, v in o.items() if k != 'workspace'}

        b = _twice(backward, ctx)
        keep = fw[r]['y'].view(split[r], C) > 0
        assert torch.equal(b['dres'].view(split[r], C), torch.where(keep, dys[r], torch.zeros_like(dys[r]))), '%s: dres' % ctx
        if is_int:
            assert torch.equal(b['dbeta'].cpu().double(), local['dbeta']), '%s: local dbeta differs from the exact sum' % ctx
        else:
            _close(b['dbeta'], local['dbeta'], bc.TOL_DPARAM, 'local dbeta', ctx, atol_rel=True)
        _close(b['dgamma'], local['dgamma'], bc.TOL_DPARAM, 'local dgamma', ctx, atol_rel=True)
        _close(b['dx'].view(split[r], C), whole['dx'][sl], (bc.TOL_DX[0], bc.TOL_DX[1] * float(whole['dx'].abs().max()) + 1e-7), 'dx', ctx)


# ---- the stem: BatchNorm -> ReLU -> MaxPool2d ------------------------------------------------------------------------------------------------------
def test_stem_refuses_c12():
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    C, N, H, W = bc.STEM_REFUSED_C, 2, 15, 13
    P, Q = bc.pool_out(H, 3, 2, 1), bc.pool_out(W, 3, 2, 1)
    x = torch.zeros(N * H * W * C, device=DEV)
    y, idx, v = _nan(N * P * Q * C), Guarded(N * P * Q * C, 0, torch.uint8), _nan(C)
    ws, wsb = _workspace(lib, N * H * W, C)
    st = lib.nnl_bn_relu_maxpool_fwd(ptr(x), None, None, ptr(y.t), ptr(idx.t), ptr(v.t), ptr(v.t), ptr(v.t), ptr(v.t), None, None, N, H, W, C, P, Q,
                                     3, 2, 1, bc.EPS, bc.MOMENTUM, 1, None, ptr(ws.t), wsb, stream())
    torch.cuda.synchronize()
    assert st == -1 and bc.STEM_REFUSAL in lib.nnl_last_error()
    assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(v.t).all()) and bool(torch.isnan(ws.t).all())


def test_stem_backward_refuses_geometry_the_forward_refuses():
    """nnl_bn_relu_maxpool_bwd indexes idx and dpool by P and Q as the caller states them: a Q one larger than the pooling yields, or a
    window of 16 x 16 (kh*ks + kw no longer fits idx's byte), is refused on the host like in the forward: nothing is launched."""
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    N, H, W, C = 2, 15, 13, 16
    P, Q = bc.pool_out(H, 3, 2, 1), bc.pool_out(W, 3, 2, 1)
    npool = N * P * (Q + 1) * C
    x, dpool = torch.zeros(N * H * W * C, device=DEV), torch.zeros(npool, device=DEV)
    idx, v = torch.zeros(npool, dtype=torch.uint8, device=DEV), torch.ones(C, device=DEV)
    dx, dg, db = _nan(N * H * W * C), _nan(C), _nan(C)
    ws, wsb = _workspace(lib, N * H * W, C)
    for q, ks in ((Q + 1, 3), (Q, 16)):
        st = lib.nnl_bn_relu_maxpool_bwd(ptr(dpool), None, ptr(idx), ptr(x), ptr(v), ptr(v), ptr(v), ptr(v), ptr(v), ptr(v), ptr(dx.t), ptr(dg.t),
                                         ptr(db.t), N, H, W, C, P, q, ks, 2, 1, 1, ptr(ws.t), wsb, stream())
        err = lib.nnl_last_error()
        assert st == -1 and (b'bad geometry' in err or b'P/Q do not match' in err), 'Q=%d ks=%d: status %d: %s' % (q, ks, st, err.decode())
        assert b'bn_relu_maxpool_bwd' in err
    torch.cuda.synchronize()
    for g in (dx, dg, db, ws):
        assert bool(torch.isnan(g.t).all()) and g.intact()


STEM_SWEEP = [(c, t) for c in bc.STEM_CASES for t in ((1, 0) if c[3] == 16 else (1,))]


@pytest.mark.parametrize('case,training', STEM_SWEEP, ids=['%dx%dx%dx%d-k%ds%dp%d-%s' % (c + ('train' if t else 'eval',)) for c, t in STEM_SWEEP])
def test_stem(case, training):
    from neuralnetworklibrary_amd._lib import lib, ptr, stream
    N, H, W, C, ks, stride, pad = case
    P, Q = bc.pool_out(H, ks, stride, pad), bc.pool_out(W, ks, stride, pad)
    rows, nel, npool = N * H * W, N * H * W * C, N * P * Q * C
    ctx = 'stem %s %s' % (case, 'train' if training else 'eval')
    g = torch.Generator().manual_seed(C + H + ks)
    x = torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3
    x[:, ::3, ::2, :] = x[:, ::3, ::2, :].round()                     # ties and exact zeros after the ReLU
    gam, bet = torch.linspace(0.5, 1.5, C), torch.linspace(-0.4, 0.4, C)
    gam[:3] = torch.tensor([1e-3, 0.0, -0.7])                          # tiny / zero / negative gamma: the backward's slow and sign paths
    rm0, rv0 = torch.linspace(-0.2, 0.5, C), torch.linspace(0.8, 2.5, C)
    dpool = torch.randn(N, P, Q, C, generator=g)
    xd, gamma, beta, dpool_d = x.to(DEV), gam.to(DEV), bet.to(DEV), dpool.to(DEV)

    def forward():
        o = dict(y=_nan(npool), idx=Guarded(npool, 0xEE, torch.uint8), mean=_nan(C), invstd=_nan(C), scale=_nan(C), shift=_nan(C),
                 rmean=Guarded(C, rm0), rvar=Guarded(C, rv0), nbt=Guarded(1, 5, torch.int64))
        ws, wsb = _workspace(lib, rows, C)
        o['workspace'] = ws
        p = lambda k: ptr(o[k].t)
        st = lib.nnl_bn_relu_maxpool_fwd(ptr(xd), ptr(gamma), ptr(beta), p('y'), p('idx'), p('mean'), p('invstd'), p('scale'), p('shift'),
                                         p('rmean'), p('rvar'), N, H, W, C, P, Q, ks, stride, pad, bc.EPS, bc.MOMENTUM, training, p('nbt'),
                                         ptr(ws.t), wsb, stream())
        torch.cuda.synchronize()
        assert st == 0, '%s: status %d: %s' % (ctx, st, lib.nnl_last_error().decode())
        _check_bands(o, ctx)
        return {k: v.t for k, v in o.items() if k != 'workspace'}

    f = _twice(forward, ctx + ' fwd')
    x64 = x.double().view(rows, C)
    if training:
        mean64, var64 = bc.batch_stats(x64)
        _close(f['rmean'], bc.running_update(rm0.double(), mean64, bc.MOM32), bc.TOL_RMEAN, 'running_mean', ctx)
        _close(f['rvar'], bc.running_update(rv0.double(), bc.unbiased(var64, float(rows)), bc.MOM32), bc.TOL_RVAR, 'running_var', ctx)
        assert int(f['nbt']) == 6
    else:
        mean64, var64 = rm0.double(), rv0.double()
        assert torch.equal(f['rmean'].cpu(), rm0) and torch.equal(f['rvar'].cpu(), rv0) and int(f['nbt']) == 5
    invstd64 = 1.0 / torch.sqrt(var64 + bc.EPS32)
    _close(f['mean'], mean64, bc.TOL_RMEAN, 'save_mean', ctx)
    _close(f['invstd'], invstd64, bc.TOL_RVAR, 'save_invstd', ctx)
    scale64 = gam.double() * invstd64
    _close(f['scale'], scale64, bc.TOL_RVAR, 'save_scale', ctx)
    _close(f['shift'], bet.double() - mean64 * scale64, bc.TOL_Y, 'save_shift', ctx)

    # the forward, bit for bit: the same two fp32 operations from the kernel's own scale / shift, pooled by torch
    z, y_cpu, idx_cpu = bc.stem_forward_fp32(x, f['scale'].cpu(), f['shift'].cpu(), ks, stride, pad)
    y, idx = f['y'].view(N, P, Q, C), f['idx'].view(N, P, Q, C)
    _written(y, 'y', ctx)
    assert torch.equal(y.cpu(), y_cpu), '%s: y differs from relu(x*scale + shift) pooled, at %d elements' % (ctx, int((y.cpu() != y_cpu).sum()))
    assert torch.equal(idx.cpu(), idx_cpu), '%s: idx differs from torch\'s arg-max at %d elements' % (ctx, int((idx.cpu() != idx_cpu).sum()))
    y64 = torch.nn.functional.max_pool2d(torch.relu(x64 * scale64 + (bet.double() - mean64 * scale64)).view(N, H, W, C).permute(0, 3, 1, 2),
                                         ks, stride, pad).permute(0, 2, 3, 1)
    _close(y, y64, bc.TOL_Y, 'y vs fp64', ctx)

    # the backward against fp64 from that idx: once over the pooled outputs (y given), once over the inputs (y = NULL)
    gin = bc.stem_scatter(dpool, idx_cpu, z, H, W, ks, stride, pad).view(rows, C)
    ref = bc.bn_bwd_ref(gin, None, x64, gam.double(), mean64, invstd64, bool(training))
    outs = {}
    for with_y in (True, False):
        c2 = '%s bwd %s' % (ctx, 'with y' if with_y else 'y = NULL')

        def backward():
            o = dict(dx=_nan(nel), dgamma=_nan(C), dbeta=_nan(C))
            ws, wsb = _workspace(lib, rows, C)
            o['workspace'] = ws
            p = lambda k: ptr(o[k].t)
            st = lib.nnl_bn_relu_maxpool_bwd(ptr(dpool_d), ptr(f['y']) if with_y else None, ptr(f['idx']), ptr(xd), ptr(gamma), ptr(beta),
                                             ptr(f['mean']), ptr(f['invstd']), ptr(f['scale']), ptr(f['shift']), p('dx'), p('dgamma'), p('dbeta'),
                                             N, H, W, C, P, Q, ks, stride, pad, training, ptr(ws.t), wsb, stream())
            torch.cuda.synchronize()
            assert st == 0, '%s: status %d: %s' % (c2, st, lib.nnl_last_error().decode())
            _check_bands(o, c2)
            return {k: v.t for k, v in o.items() if k != 'workspace'}

        b = _twice(backward, c2)
        outs[with_y] = b
        _close(b['dgamma'], ref['dgamma'], bc.TOL_STEM_DPARAM, 'dgamma', c2)
        _close(b['dbeta'], ref['dbeta'], bc.TOL_DPARAM, 'dbeta', c2, atol_rel=True)
        _close(b['dx'].view(rows, C), ref['dx'], bc.TOL_DX, 'dx', c2, atol_rel=True, atol_add=1e-7)
    for k in ('dgamma', 'dbeta'):
        _close(outs[True][k], outs[False][k].double().cpu(), bc.TOL_STEM_AGREE, k + ': the two reductions', ctx)
    _close(outs[True]['dx'], outs[False]['dx'].double().cpu(), (1e-4, 1e-5 * float(ref['dx'].abs().max())), 'dx: the two reductions', ctx)
