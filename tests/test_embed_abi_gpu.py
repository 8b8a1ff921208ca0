"""The tabular and collab embedding C ABI (csrc/tabular.hip, csrc/embdotbias.hip, csrc/linear_small.hip; include/nnl.h) called directly over
the launch regimes and routes of tests/embed_cases.py, against its fp64 references: `int` data bit for bit on every route, `randn` data
within the counted bounds, the route taken asserted from the route note of the call.

Around every call: each output sits between two bands of sentinel values and is pre-filled with NaN (an element the kernel leaves
unwritten shows), a workspace has exactly the documented size between bands, the inputs are compared with what was uploaded, and the call
is repeated from the same state and must reproduce itself bit for bit (the atomic routes in `randn` mode alone are exempt).  The embedding
tables of the collab calls sit inside NaN arenas, so that a read of row -1 or of row `card` shows.  Every out-of-range index here is one
the kernels are documented to skip.  Every test prints max err / bound.
"""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

import embed_cases as ec

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 1024
SENT = np.float32(12345.0)
F32 = np.float32
ERR_ARG, ERR_WORKSPACE = -1, -4


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


def _abi():
    from neuralnetworklibrary_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream


class Band:
    """n elements between two bands of GUARD sentinels in one allocation; the n elements start as NaN (float32) or -7 (integers)"""

    def __init__(self, n, dtype=torch.float32, fill=None):
        self.n, self.dtype = int(n), dtype
        self.sent = float(SENT) if dtype == torch.float32 else 777
        self.buf = torch.full((self.n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + self.n]
        self.view.fill_(fill if fill is not None else (float('nan') if dtype == torch.float32 else -7))

    def get(self, what, ctx):
        a = self.buf.cpu().numpy()
        assert (a[:GUARD] == self.sent).all() and (a[GUARD + self.n:] == self.sent).all(), '%s: wrote outside %s (sentinel touched)' % (ctx, what)
        return a[GUARD:GUARD + self.n].copy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _unchanged(dev, host, what, ctx):
    if dev is not None:
        assert np.array_equal(dev.cpu().numpy().view(np.uint8).ravel(), np.ascontiguousarray(host).view(np.uint8).ravel()), \
            '%s: input %s was written' % (ctx, what)


def _same(a, b):
    raw = lambda v: np.atleast_1d(np.asarray(v)).view(np.uint8)
    return all(np.array_equal(raw(a[k]), raw(b[k])) for k in a if a[k] is not None)


def _twice(run, ctx, *a):
    one, two = run(*a, ctx), run(*a, ctx)
    assert _same(one, two), '%s: two calls from the same state differ (not bitwise reproducible)' % ctx
    return one


def _notes(lib, call):
    "(status, the route notes of the call)"
    buf = ctypes.create_string_buffer(16384)
    lib.nnl_debug_route_record(1)
    try:
        st = call()
        assert lib.nnl_debug_route_collect(buf, len(buf)) >= 0
    finally:
        lib.nnl_debug_route_record(0)
    return st, [n for n in buf.value.decode().split(';') if n]


def _note_arr(notes):
    return np.frombuffer(';'.join(notes).encode().ljust(96), dtype=np.uint8)


def _note(got):
    return got['note'].tobytes().decode().strip()


class Env:
    "sets library switches for a block and puts the environment back, every site reading it again"

    def __init__(self, env):
        self.env = dict(env or {})

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        if self.env:
            os.environ.update(self.env)
            _abi()[1].nnl_reload_env()

    def __exit__(self, *exc):
        if not self.env:
            return
        _, lib, _, _ = _abi()
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.nnl_reload_env()


class Arena:
    "a [rows, D] table inside a NaN-filled allocation: the rows before and behind it read as NaN"

    def __init__(self, w, margin=4):
        rows, D = w.shape
        self.buf = torch.full(((rows + 2 * margin) * D,), float('nan'), dtype=torch.float32, device=DEV)
        self.view = self.buf[margin * D:(margin + rows) * D]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(w)).reshape(-1))
        self.host = w

    def unchanged(self, what, ctx):
        _unchanged(self.view, self.host, what, ctx)


# ---- the tabular front end ------------------------------------------------------------------------------------------------------------------
class TabDev:
    "the device side of one tabular case: tables, descriptor arrays, masks"

    def __init__(self, d):
        L, case = d['L'], d['case']
        self.d, self.L, self.case = d, L, case
        self.tables = [_dev(w) for w in d['tables']]
        self.ptrs = _dev(np.asarray([t.data_ptr() for t in self.tables] or [0], dtype=np.int64))
        for k in ('card', 'dim', 'col_off', 'row_off', 'grad_off', 'col_table', 'row_table', 'blk_col', 'blk_first'):
            a = L[k]
            setattr(self, k, _dev(a if a.size else np.zeros(1, dtype=a.dtype)))
        self.x = _dev(d['x'] if d['x'].size else np.zeros((1, 1), dtype=np.int64))
        self.row_mask, self.cont, self.cont_mask, self.dout = _dev(d['row_mask']), _dev(d['cont']), _dev(d['cont_mask']), _dev(d['dout'])

    def inputs_unchanged(self, ctx):
        d = self.d
        for w, h in zip(self.tables, d['tables']):
            _unchanged(w, h, 'a table', ctx)
        if d['x'].size:
            _unchanged(self.x, d['x'], 'xcat', ctx)
        for dev, host, what in ((self.row_mask, d['row_mask'], 'row_mask'), (self.cont, d['cont'], 'cont'),
                                (self.cont_mask, d['cont_mask'], 'cont_mask'), (self.dout, d['dout'], 'dout')):
            _unchanged(dev, host, what, ctx)


def run_gather(d, ctx):
    check, lib, ptr, stream = _abi()
    t, L, case = TabDev(d), d['L'], d['case']
    ncat, ld = len(case.cards), L['cat_width'] + case.n_cont + case.pad
    out = Band(case.bs * ld)
    p = (lambda a: ptr(a)) if ncat else (lambda a: None)
    st, notes = _notes(lib, lambda: lib.nnl_tab_gather_fwd(p(t.x), p(t.ptrs), p(t.card), p(t.dim), p(t.col_off), p(t.col_table), ptr(t.row_mask),
                                                          ptr(t.cont), ptr(t.cont_mask), ptr(out.view), case.bs, ncat, L['cat_width'], case.n_cont,
                                                          ld, stream()))
    check(st)
    torch.cuda.synchronize()
    t.inputs_unchanged(ctx)
    return dict(out=out.get('out', ctx).reshape(case.bs, ld), note=_note_arr(notes))


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('case', ec.GATHER_CASES, ids=ec.case_id)
def test_tab_gather(case, mode):
    d = ec.tab_data(case, mode)
    ctx = 'gather-%s-%s' % (case.name, mode)
    got = _twice(run_gather, ctx, d)
    assert _note(got) == ('' if case.bs == 0 else 'tab_gather'), _note(got)
    ec.check_tab_fwd(d, got['out'], ctx)
    _say('RATIO %-24s bit for bit (%s)' % (ctx, _note(got) or 'bs = 0: no launch'))


BWD_ROUTES = ('scan', 'det', 'atomic-null', 'atomic-short', 'atomic-env')


def run_tab_bwd(d, route, ctx):
    check, lib, ptr, stream = _abi()
    t, L, case = TabDev(d), d['L'], d['case']
    bs, ncat, ld = case.bs, len(case.cards), L['cat_width'] + case.n_cont + case.pad
    dtab = Band(L['grad_elems'])
    dcont = Band(bs * case.n_cont) if case.n_cont and case.dcont else None
    pc = ptr(dcont.view) if dcont is not None else None
    wsb = int(lib.nnl_tab_scatter_bwd_workspace_bytes(bs, ncat))
    assert wsb == 4 * bs * ncat
    ws = Band(wsb // 4, torch.int32)
    if route == 'scan':
        call = lambda: lib.nnl_tab_scan_bwd(ptr(t.x), ptr(t.card), ptr(t.dim), ptr(t.col_off), ptr(t.grad_off), ptr(t.row_mask), ptr(t.cont_mask),
                                            ptr(t.dout), ptr(dtab.view), pc, ptr(t.blk_col), ptr(t.blk_first), L['n_scan'], max(case.dims), bs,
                                            ncat, L['cat_width'], case.n_cont, ld, stream())
    else:
        w, b = {'det': (ptr(ws.view), wsb), 'atomic-null': (None, wsb), 'atomic-short': (ptr(ws.view), wsb - 4),
                'atomic-env': (ptr(ws.view), wsb)}[route]
        call = lambda: lib.nnl_tab_scatter_bwd(ptr(t.x), ptr(t.card), ptr(t.dim), ptr(t.col_off), ptr(t.col_table), ptr(t.grad_off),
                                               ptr(t.row_mask), ptr(t.cont_mask), ptr(t.dout), ptr(dtab.view), L['grad_elems'], pc, bs, ncat,
                                               L['cat_width'], case.n_cont, ld, w, b, stream())
    with Env({'NNL_SCATTER_ATOMIC': '1'} if route == 'atomic-env' else {}):
        st, notes = _notes(lib, call)
    check(st)
    torch.cuda.synchronize()
    t.inputs_unchanged(ctx)
    ws.get('the sort workspace', ctx)
    return dict(dtab=dtab.get('dtab_flat', ctx), dcont=None if dcont is None else dcont.get('dcont', ctx).reshape(bs, case.n_cont),
                note=_note_arr(notes))


def tab_bwd_note(case, route):
    L = ec.tab_layout(case)
    if route == 'scan':
        return 'tab_scan_bwd@blocks=%d+%d' % (L['n_scan'], ec.cdiv(case.bs * case.n_cont, 256) if case.n_cont and case.dcont else 0)
    return 'tab_scatter_bwd<det>' if route == 'det' and case.bs <= ec.DET_MAX else 'tab_scatter_bwd<atomic>'


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('route', BWD_ROUTES)
@pytest.mark.parametrize('case', ec.BWD_CASES, ids=ec.case_id)
def test_tab_backward(case, route, mode):
    d = ec.tab_data(case, mode)
    ctx = 'tab_bwd-%s-%s-%s' % (case.name, route, mode)
    want_note = tab_bwd_note(case, route)
    if 'atomic' in want_note and mode == 'randn':
        got = run_tab_bwd(d, route, ctx)                                     # fp32 atomics in arrival order: no two runs alike
    else:
        got = _twice(run_tab_bwd, ctx, d, route)
    assert _note(got) == want_note, '%s: route %r, want %r' % (ctx, _note(got), want_note)
    r = ec.check_tab_bwd(d, got['dtab'], got['dcont'], ctx)
    _say('RATIO %-36s dtab %.3f  (%s)' % (ctx, r, want_note))
    assert r <= 1.0


def test_tab_scan_refuses_a_width_above_32():
    check, lib, ptr, stream = _abi()
    case = ec.TabCase('w33', 8, (5,), (33,), 0, 0, False, False, False, False, [])
    d = ec.tab_data(case, 'randn')
    t, L = TabDev(d), d['L']
    dtab = Band(L['grad_elems'])
    st, notes = _notes(lib, lambda: lib.nnl_tab_scan_bwd(ptr(t.x), ptr(t.card), ptr(t.dim), ptr(t.col_off), ptr(t.grad_off), None, None, ptr(t.dout),
                                                        ptr(dtab.view), None, ptr(t.blk_col), ptr(t.blk_first), L['n_scan'], 33, 8, 1, 33, 0, 33,
                                                        stream()))
    assert st == ERR_ARG and b'tab_scan_bwd' in lib.nnl_last_error() and notes == []
    torch.cuda.synchronize()
    assert np.isnan(dtab.get('dtab_flat', 'max_dim = 33')).all(), 'something ran'
    got = run_tab_bwd(d, 'det', 'w33-det')                                   # the route such a table takes instead
    assert _note(got) == 'tab_scatter_bwd<det>' and ec.check_tab_bwd(d, got['dtab'], None, 'w33-det') <= 1.0


def run_renorm(d, ctx):
    check, lib, ptr, stream = _abi()
    case = d['case']
    L = ec.tab_layout(case)
    tables = [_dev(w) for w in d['tables']]
    ptrs = _dev(np.asarray([t.data_ptr() for t in tables], dtype=np.int64))
    dev = {k: _dev(L[k]) for k in ('card', 'dim', 'row_off', 'row_table')}
    x = _dev(d['x'] if d['x'].size else np.zeros((1, len(case.cards)), dtype=np.int64))
    flags, err = Band(L['total_rows'], torch.int32, fill=0), Band(1, torch.int32, fill=0)
    st, notes = _notes(lib, lambda: lib.nnl_tab_renorm(ptr(x), ptr(ptrs), ptr(dev['card']), ptr(dev['dim']), ptr(dev['row_off']),
                                                      ptr(dev['row_table']), ptr(flags.view), case.bs, len(case.cards), L['total_rows'],
                                                      ec.MAX_NORM, ptr(err.view), stream()))
    check(st)
    torch.cuda.synchronize()
    if d['x'].size:
        _unchanged(x, d['x'], 'xcat', ctx)
    out = dict(flags=flags.get('flags', ctx), err=err.get('err_flag', ctx), note=_note_arr(notes))
    for j, t in enumerate(tables):
        out['table%d' % j] = t.cpu().numpy()
    return out


@pytest.mark.parametrize('case', ec.RENORM_CASES, ids=ec.case_id)
def test_tab_renorm(case):
    d = ec.renorm_data(case)
    ctx = 'renorm-' + case.name
    got = _twice(run_renorm, ctx, d)
    assert _note(got) == ('' if case.bs == 0 else 'tab_renorm'), _note(got)
    r = ec.check_renorm(d, [got['table%d' % j] for j in range(len(case.cards))], got['err'][0], got['flags'], ctx)
    _say('RATIO %-24s scaled rows %.3f' % (ctx, r))
    assert r <= 1.0


def _fake_ctx(xcat, row_mask, cont_mask, plan, n_cont):
    return types.SimpleNamespace(saved_tensors=(xcat, row_mask, cont_mask), plan=plan, n_cont=n_cont,
                                 needs_input_grad=(False, True, False, False, False, False) + (True,) * plan.ncat)


@pytest.mark.parametrize('which', ['default', 'max_dim33', 'NNL_TAB_SCAN=0', 'above2^28'])
def test_python_selection_of_the_tabular_backward(which):
    """_TabEmbedConcat.backward picks the scan unless a table is wider than 32, NNL_TAB_SCAN=0 or gradient elements x samples exceed 2^28;
    called on this thread (route notes are per thread), against the fp64 reference"""
    from neuralnetworklibrary_amd import ops
    _, lib, _, _ = _abi()
    if which == 'max_dim33':
        case = ec.TabCase(which, 64, (9, 7), (33, 2), 3, 0, True, True, True, True, [])
    elif which == 'above2^28':
        case = ec.TabCase(which, 1024, (70000,), (4,), 0, 0, False, False, False, False, [])
    else:
        case = ec.TabCase(which, 64, (9, 7), (5, 2), 3, 0, True, True, True, True, [])
    d = ec.tab_data(case, 'int')
    L = d['L']
    assert (L['grad_elems'] * case.bs > 2 ** 28) == (which == 'above2^28') and L['grad_elems'] * case.bs < 2 ** 28 + 2 ** 25
    weights = [_dev(w) for w in d['tables']]
    plan = ops.TabularPlan(weights)
    ctx = _fake_ctx(_dev(d['x']), _dev(d['row_mask']), _dev(d['cont_mask']), plan, case.n_cont)
    with Env({'NNL_TAB_SCAN': '0'} if which == 'NNL_TAB_SCAN=0' else {}):
        _, notes = _notes(lib, lambda: ctx.__setattr__('grads', ops._TabEmbedConcat.backward(ctx, _dev(d['dout']))))
    torch.cuda.synchronize()
    want = 'tab_scan_bwd@blocks=%d+%d' % (L['n_scan'], ec.cdiv(case.bs * case.n_cont, 256)) if which == 'default' else 'tab_scatter_bwd<det>'
    assert notes == [want], notes
    grads = ctx.grads
    dtab = np.concatenate([g.cpu().numpy().ravel() for g in grads[6:]])
    assert ec.check_tab_bwd(d, dtab, None if grads[1] is None else grads[1].cpu().numpy(), which) == 0.0
    _say('RATIO python selection %-16s bit for bit (%s)' % (which, want))


def test_a_bad_index_without_max_norm_is_skipped_and_not_reported():
    """the contract of include/nnl.h, pinned: nnl_tab_gather_fwd takes no flag, so tab_embed_concat(max_norm=None) returns zero columns for
    an index outside [0, card) and leaves the index-error flag alone; with max_norm the renorm pass reports it"""
    from neuralnetworklibrary_amd import ops
    case = ec.TabCase('quiet', 64, (9, 7), (5, 2), 0, 0, False, False, False, True, [])
    d = ec.tab_data(case, 'randn')
    weights = [_dev(w) for w in d['tables']]
    flag = ops.index_error_flag(weights[0].device)
    flag.zero_()
    out, _ = ops.tab_embed_concat(_dev(d['x']), weights, max_norm=None)
    ec.check_tab_fwd(d, out.cpu().numpy(), 'quiet')
    assert int(flag.item()) == 0
    ops.tab_embed_concat(_dev(d['x']), weights, max_norm=100.0)              # (no row is that long: the tables stay as they are)
    assert int(flag.item()) == 1
    flag.zero_()


# ---- EmbeddingDotBias -----------------------------------------------------------------------------------------------------------------------
def run_ed(d, ctx):
    check, lib, ptr, stream = _abi()
    case = d['case']
    n, nu, ni, D = case.n, case.n_user, case.n_item, case.D
    x = _dev(d['x'] if n else np.zeros((1, 2), dtype=np.int64))
    Ua, Ma = Arena(d['U']), Arena(d['M'])
    bu, bi = Arena(d['bu'][:, None]), Arena(d['bi'][:, None])
    z_in, dy = _dev(d['z'] if n else np.zeros(1, dtype=F32)), _dev(d['dy'] if n else np.zeros(1, dtype=F32))
    y, z = Band(n), Band(n) if case.zmode != 'none' else None
    flag = Band(1, torch.int32, fill=0) if case.err_flag else None
    with Env(case.env):
        st, fnotes = _notes(lib, lambda: lib.nnl_embdotbias_fwd(ptr(x), ptr(Ua.view), ptr(Ma.view), ptr(bu.view), ptr(bi.view), ptr(y.view),
                                                               None if z is None else ptr(z.view), n, nu, ni, D, case.has_range, ec.ED_LO,
                                                               ec.ED_HI, None if flag is None else ptr(flag.view), stream()))
        check(st)
        sizes = (nu * D, ni * D, nu, ni)
        if case.layout == 'block':
            block = Band(sum(sizes))
            offs = np.concatenate([[0], np.cumsum(sizes)])
            views = [block.view[offs[k]:offs[k + 1]] for k in range(4)]
            bands = [block]
        else:
            bands = [Band(s) for s in sizes]
            views = [b.view for b in bands]
        wsb = int(lib.nnl_embdotbias_bwd_workspace_bytes(n))
        assert wsb == 12 * n
        ws = Band(wsb // 4, torch.int32)
        st, notes = _notes(lib, lambda: lib.nnl_embdotbias_bwd(ptr(x), ptr(Ua.view), ptr(Ma.view), ptr(z_in), ptr(dy), ptr(views[0]), ptr(views[1]),
                                                              ptr(views[2]), ptr(views[3]), n, nu, ni, D, case.has_range, ec.ED_LO, ec.ED_HI,
                                                              ptr(ws.view) if case.ws == 'full' else None, wsb, stream()))
        check(st)
    torch.cuda.synchronize()
    for a, what in ((Ua, 'U'), (Ma, 'M'), (bu, 'bu'), (bi, 'bi')):
        a.unchanged(what, ctx)
    if n:
        _unchanged(x, d['x'], 'x', ctx)
        _unchanged(z_in, d['z'], 'z', ctx)
        _unchanged(dy, d['dy'], 'dy', ctx)
    ws.get('the workspace', ctx)
    if case.layout == 'block':
        flat = block.get('[dU | dM | dbu | dbi]', ctx)
        outs = [flat[offs[k]:offs[k + 1]] for k in range(4)]
    else:
        outs = [b.get(k, ctx) for b, k in zip(bands, ('dU', 'dM', 'dbu', 'dbi'))]
    return dict(y=y.get('y', ctx), z=None if z is None else z.get('z', ctx), flag=None if flag is None else flag.get('err_flag', ctx),
                dU=outs[0], dM=outs[1], dbu=outs[2], dbi=outs[3], note=_note_arr(fnotes + notes))


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('case', ec.ED_CASES, ids=ec.case_id)
def test_embdotbias(case, mode):
    d = ec.ed_data(case, mode)
    ctx = 'embdot-%s-%s' % (case.name, mode)
    route = ec.ed_route(case)
    if route and 'atomic' in route and mode == 'randn':
        got = run_ed(d, ctx)
    else:
        got = _twice(run_ed, ctx, d)
    want = ';'.join(n for n in ('embdot_fwd' if case.n else None, route) if n)
    assert _note(got) == want, '%s: route %r, want %r' % (ctx, _note(got), want)
    r = ec.check_ed_fwd(d, got['y'], got['z'], None if got['flag'] is None else got['flag'][0], ctx)
    rb = ec.check_ed_bwd(d, got, ctx)
    _say('RATIO %-30s %s  %s  (%s)' % (ctx, ec.fmt_ratios(r), ec.fmt_ratios(rb), route or 'n = 0: fills only'))
    assert max(list(r.values()) + list(rb.values())) <= 1.0


# ---- the small linear layer -------------------------------------------------------------------------------------------------------------------
def run_lin(d, short_ws, ctx):
    check, lib, ptr, stream = _abi()
    c = d['case']
    M, K, N, ldx = c.M, c.K, c.N, c.K + c.ldx_pad
    x = _dev(d['x'] if M else np.zeros((1, ldx), dtype=F32))
    w, b, dy = _dev(d['w']), _dev(d['b']), _dev(d['dy'] if M else np.zeros((1, N), dtype=F32))
    y = Band(M * N)
    st, fnotes = _notes(lib, lambda: lib.nnl_linear_small_fwd(ptr(x), ptr(w), ptr(b), ptr(y.view), M, K, ldx, N, stream()))
    check(st)
    outs = {k: Band(n) if k in c.outs else None for k, n in (('dx', M * K), ('dw', N * K), ('db', N))}
    p = lambda k: None if outs[k] is None else ptr(outs[k].view)
    need = 'dw' in c.outs or 'db' in c.outs
    wsb = int(lib.nnl_linear_small_bwd_workspace_bytes(M, K, N))
    assert wsb == 4 * ec.cdiv(M, ec.LIN_SLAB) * N * (K + 1)
    ws = Band(wsb // 4)
    st, notes = _notes(lib, lambda: lib.nnl_linear_small_bwd(ptr(dy), ptr(x), ptr(w), p('dx'), p('dw'), p('db'), M, K, ldx, N,
                                                            ptr(ws.view) if need else None, wsb - 4 if short_ws else wsb if need else 0, stream()))
    torch.cuda.synchronize()
    if M:
        _unchanged(x, d['x'], 'x', ctx)
        _unchanged(dy, d['dy'], 'dy', ctx)
    _unchanged(w, d['w'], 'w', ctx)
    _unchanged(b, d['b'], 'bias', ctx)
    ws.get('the workspace', ctx)
    got = dict(y=y.get('y', ctx).reshape(M, N), status=np.asarray([st]), note=_note_arr(fnotes + notes))
    for k, band in outs.items():
        got[k] = None if band is None else band.get(k, ctx)
    return got


@pytest.mark.parametrize('mode', ec.MODES)
@pytest.mark.parametrize('case', ec.LIN_CASES, ids=ec.case_id)
def test_linear_small(case, mode):
    d = ec.lin_data(case, mode)
    ctx = 'linear-%s-%s' % (case.name, mode)
    got = _twice(run_lin, ctx, d, False)
    assert got['status'][0] == 0
    nslab = ec.cdiv(case.M, ec.LIN_SLAB) if ('dw' in case.outs or 'db' in case.outs) else 0
    want = 'linear_small_fwd;linear_small_bwd:%s@slabs=%d' % (case.outs, nslab) if case.M else ''
    assert _note(got) == want, '%s: route %r, want %r' % (ctx, _note(got), want)
    r = ec.check_lin(d, got, ctx)
    _say('RATIO %-24s %s' % (ctx, ec.fmt_ratios(r)))
    assert max(r.values()) <= 1.0


def test_linear_small_short_workspace_and_five_outputs():
    check, lib, ptr, stream = _abi()
    d = ec.lin_data(next(c for c in ec.LIN_CASES if c.name == 'm65-all'), 'randn')
    got = run_lin(d, True, 'linear-short-ws')
    assert got['status'][0] == ERR_WORKSPACE and b'linear_small_bwd' in lib.nnl_last_error()
    assert _note(got) == 'linear_small_fwd', _note(got)
    for k in ('dx', 'dw', 'db'):
        assert np.isnan(got[k]).all(), 'a short workspace, yet %s was written' % k
    f = Band(64)
    p = ptr(f.view)
    assert lib.nnl_linear_small_supported(4) == 1 and lib.nnl_linear_small_supported(5) == 0
    for call in (lambda: lib.nnl_linear_small_fwd(p, p, p, p, 2, 4, 4, 5, stream()),
                 lambda: lib.nnl_linear_small_bwd(p, p, p, p, p, p, 2, 4, 4, 5, p, 256, stream()),
                 lambda: lib.nnl_linear_small_fwd(p, p, p, p, 2, 4, 3, 1, stream())):                      # ldx < K
        st, notes = _notes(lib, call)
        assert st == ERR_ARG and notes == []
    torch.cuda.synchronize()
    assert np.isnan(f.get('the operand', 'N = 5')).all()


# ---- pad_cols, keep_masks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ec.PAD_CASES, ids=ec.case_id)
def test_pad_cols(case):
    check, lib, ptr, stream = _abi()
    src = ec.pad_data(case)
    s = _dev(src if case.rows else np.zeros((1, case.C), dtype=F32))
    dst = Band(case.rows * case.Cp)
    check(lib.nnl_pad_cols(ptr(s), ptr(dst.view), case.rows, case.C, case.Cp, stream()))
    torch.cuda.synchronize()
    ec.check_pad(case, src, dst.get('dst', case.name), case.name)
    if case.rows:
        _unchanged(s, src, 'src', case.name)


@pytest.mark.parametrize('case', ec.KEEP_CASES, ids=ec.case_id)
def test_keep_masks(case):
    check, lib, ptr, stream = _abi()
    u = ec.keep_data(case)
    du = _dev(u)
    a, b = Band(case.na), Band(case.nb)
    check(lib.nnl_keep_masks(ptr(du), ptr(a.view) if case.na else None, case.na, case.keep_a, ptr(b.view) if case.nb else None, case.nb,
                             case.keep_b, stream()))
    torch.cuda.synchronize()
    _unchanged(du, u, 'u', case.name)
    ec.check_keep(case, u, a.get('a', case.name), b.get('b', case.name), case.name)
