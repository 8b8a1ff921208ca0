"""The text-loss C ABI (csrc/text.hip: nnl_softmax_ce_fwd / _bwd, nnl_embedding_rowmask_fwd / _bwd, nnl_seq_reg_fwd / _bwd,
nnl_weight_drop and the two workspace queries; include/nnl.h) called directly over the launch regimes of its kernels, against the fp64
references of tests/text_cases.py, and the wrappers on top of it (ops.cross_entropy_nd over its three layout branches, the padded
gradient hand-over) against F.cross_entropy in fp64 on the CPU.

Around every call: each output sits between two bands of sentinel values and is pre-filled with NaN (an element the kernel leaves
unwritten shows), a workspace has exactly the documented size between bands, the inputs are compared with what was uploaded, and the call
is repeated from the same state and must reproduce itself bit for bit (the atomic embedding backward in `randn` mode alone is exempt).
Every test prints max err / bound.
"""
import ctypes
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import text_cases as tc
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 1024
SENT = np.float32(12345.0)
F32 = np.float32


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


def _abi():
    from neuralnetworklibrary_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream


class Band:
    """n elements between two bands of GUARD sentinels in one allocation; the n elements start as NaN (float32) or -7 (int32)"""

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
        assert np.array_equal(dev.cpu().numpy().view(np.uint8), np.ascontiguousarray(host).view(np.uint8)), '%s: input %s was written' % (ctx, what)


def _same(a, b):
    raw = lambda v: np.atleast_1d(np.asarray(v)).view(np.uint8)
    return all(np.array_equal(raw(a[k]), raw(b[k])) for k in a)


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


# ---- softmax-CE -----------------------------------------------------------------------------------------------------------------------------
def run_ce(case, x, t, ctx):
    check, lib, ptr, stream = _abi()
    rows, V, ld = case.rows, case.V, tc.ce_ld(case.V, case.ld)
    d_x, d_t, d_g = _dev(x), _dev(t), _dev(np.asarray([case.gout], dtype=F32))
    stats, loss, mean, dl = Band(2 * rows), Band(rows), Band(1), Band(rows * ld)
    flag = Band(1, torch.int32, fill=0)
    check(lib.nnl_softmax_ce_fwd(ptr(d_x), ptr(d_t), ptr(stats.view), ptr(loss.view), ptr(mean.view), rows, V, ptr(flag.view), stream()))
    check(lib.nnl_softmax_ce_bwd(ptr(d_x), ptr(d_t), ptr(stats.view), ptr(d_g), ptr(dl.view), rows, V, ld, stream()))
    torch.cuda.synchronize()
    _unchanged(d_x, x, 'logits', ctx)
    _unchanged(d_t, t, 'target', ctx)
    _unchanged(d_g, np.asarray([case.gout], dtype=F32), 'grad_out', ctx)
    return dict(stats=stats.get('row_stats', ctx).reshape(rows, 2), loss_rows=loss.get('loss_rows', ctx), mean=mean.get('loss_mean', ctx)[0],
                d=dl.get('dlogits', ctx).reshape(rows, ld), err_flag=flag.get('err_flag', ctx)[0])


@pytest.mark.parametrize('case', tc.CE_CASES, ids=tc.case_id)
def test_softmax_ce(case):
    x, t, masked = tc.ce_data(case)
    got = _twice(run_ce, 'ce-' + case.name, case, x, t)
    r = tc.check_ce(case, x, t, masked, got, 'ce-' + case.name)
    _say('RATIO ce %-18s %-13s %s' % (case.name, case.mode, tc.fmt_ratios(r)))
    assert max(r.values()) <= 1.0
    if case.mode == 'masked':
        assert np.isfinite(got['loss_rows']).all() and np.isfinite(got['d']).all()
    if case.mode == 'nonfinite':
        assert np.isnan(got['loss_rows'][:3]).all() and np.isfinite(got['loss_rows'][3:]).all() and np.isnan(got['mean'])
        assert np.isnan(got['d'][:3, :case.V]).all() and np.isfinite(got['d'][3:]).all()
    if case.mode == 'badtarget':
        ref = tc.ce_reference(x, t, case.gout)
        assert got['err_flag'] == 1 and not got['loss_rows'][[2, 5]].any() and got['loss_rows'][[0, 1, 3, 4, 6]].all()
        assert abs(float(got['mean']) - ref['loss'].sum() / case.rows) <= 4 * ref['loss_bound'].max()      # over ALL rows, the bad ones as 0


# ---- embedding with a row mask ------------------------------------------------------------------------------------------------------------------
def run_emb(d, ws_short, ctx):
    """forward and backward of one case; ws_short: hand the backward a workspace that is 4 bytes short.  Returns out, flag, dW and the
    route note of the backward."""
    check, lib, ptr, stream = _abi()
    x, W, rm, dout = d['x'], d['W'], d['rowmask'], d['dout']
    n, (V, D) = len(x), W.shape
    d_x, d_W, d_rm, d_dout = _dev(x), _dev(W), _dev(rm), _dev(dout)
    out, dW = Band(n * D), Band(V * D)
    flag = Band(1, torch.int32, fill=0)
    check(lib.nnl_embedding_rowmask_fwd(ptr(d_x), ptr(d_W), ptr(d_rm), ptr(out.view), n, V, D, ptr(flag.view), stream()))
    wsb = int(lib.nnl_embedding_rowmask_bwd_workspace_bytes(n))
    assert wsb == 4 * n
    ws = Band(wsb // 4, torch.int32)
    st, notes = _notes(lib, lambda: lib.nnl_embedding_rowmask_bwd(ptr(d_x), ptr(d_rm), ptr(d_dout), ptr(dW.view), n, V, D, d['pad'],
                                                                  ptr(ws.view) if wsb else None, wsb - 4 if ws_short else wsb, stream()))
    check(st)
    torch.cuda.synchronize()
    ws.get('the sort workspace', ctx)
    for dev, host, what in ((d_x, x, 'x'), (d_W, W, 'W'), (d_rm, rm, 'rowmask'), (d_dout, dout, 'dout')):
        _unchanged(dev, host, what, ctx)
    return dict(out=out.get('out', ctx).reshape(n, D), flag=flag.get('err_flag', ctx), dW=dW.get('dW', ctx).reshape(V, D),
                note=np.frombuffer(';'.join(notes).encode().ljust(64), dtype=np.uint8))


def _note(got):
    return got['note'].tobytes().decode().strip()


@pytest.mark.parametrize('mode', tc.EMB_MODES)
@pytest.mark.parametrize('case', tc.EMB_CASES, ids=tc.case_id)
def test_embedding_rowmask(case, mode):
    d = tc.emb_data(case, mode)
    ctx = 'emb-%s-%s' % (case.name, mode)
    atomic = case.n > tc.EMB_MAX_SORT
    if atomic and mode == 'randn':
        got = run_emb(d, False, ctx)                                         # fp32 atomics in arrival order: no two runs alike
    else:
        got = _twice(run_emb, ctx, d, False)
    assert _note(got) == ('' if case.n == 0 else 'emb_rowmask_bwd<atomic>' if atomic else 'emb_rowmask_bwd<det>'), _note(got)
    want, flag = tc.emb_fwd_ref(d)
    tc._same_bits(got['out'], want, 'out', ctx)
    assert int(got['flag'][0]) == flag, '%s: err_flag %r' % (ctx, got['flag'])
    r = tc.check_emb_bwd(d, got['dW'], ctx)
    _say('RATIO %-22s dW %.3f  (%s)' % (ctx, r, _note(got) or 'n = 0: memset only'))
    assert r <= 1.0


@pytest.mark.parametrize('mode', tc.EMB_MODES)
def test_embedding_backward_routes(mode, monkeypatch):
    """the three situations in which the backward takes the atomic kernel — a short workspace, n > 32768 (test_embedding_rowmask[atomic])
    and NNL_SCATTER_ATOMIC=1 — and the default; every one against the reference (`int` mode: bit for bit on either path)"""
    _, lib, _, _ = _abi()
    case = next(c for c in tc.EMB_CASES if c.name == 'd8')
    d = tc.emb_data(case, mode)
    for ws_short, env, want in ((False, None, 'emb_rowmask_bwd<det>'), (True, None, 'emb_rowmask_bwd<atomic>'),
                                (False, '1', 'emb_rowmask_bwd<atomic>'), (False, '0', 'emb_rowmask_bwd<det>')):
        if env is None:
            monkeypatch.delenv('NNL_SCATTER_ATOMIC', raising=False)
        else:
            monkeypatch.setenv('NNL_SCATTER_ATOMIC', env)
        lib.nnl_reload_env()
        ctx = 'emb-route-%s-short %s-env %s' % (mode, ws_short, env)
        got = run_emb(d, ws_short, ctx)
        assert _note(got) == want, '%s: route %r, want %r' % (ctx, _note(got), want)
        r = tc.check_emb_bwd(d, got['dW'], ctx)
        _say('RATIO %-40s dW %.3f  (%s)' % (ctx, r, want))
        assert r <= 1.0
    monkeypatch.undo()                                                       # the variable as it was, and every site reads it again
    lib.nnl_reload_env()


# ---- AR / TAR ---------------------------------------------------------------------------------------------------------------------------------
def run_reg(h, alpha, beta, g, ctx):
    check, lib, ptr, stream = _abi()
    T, R = h.shape
    d_h = _dev(h)
    d_g = None if g is None else _dev(np.asarray([g], dtype=F32))
    wsb = int(lib.nnl_seq_reg_workspace_bytes(T, R))
    assert wsb == 4 * 2 * tc.REG_MAX_BLOCKS
    ws, out3, dh = Band(wsb // 4), Band(3), Band(T * R)
    check(lib.nnl_seq_reg_fwd(ptr(d_h), ptr(out3.view), T, R, alpha, beta, ptr(ws.view), wsb, stream()))
    check(lib.nnl_seq_reg_bwd(ptr(d_h), ptr(d_g), ptr(dh.view), T, R, alpha, beta, stream()))
    torch.cuda.synchronize()
    ws.get('the workspace', ctx)
    _unchanged(d_h, h, 'h', ctx)
    return dict(out3=out3.get('out3', ctx), dh=dh.get('dh', ctx).reshape(T, R))


@pytest.mark.parametrize('mode', tc.REG_MODES)
@pytest.mark.parametrize('case', tc.REG_CASES, ids=tc.case_id)
def test_seq_reg(case, mode):
    h = tc.reg_data(case, mode)
    for (alpha, beta), g in zip(tc.REG_AB + tc.REG_AB[2:], (None, 2.5, None, 2.5)):
        ctx = 'reg-%s-%s-a%g-b%g-g%s' % (case.name, mode, alpha, beta, g)
        got = _twice(run_reg, ctx, h, alpha, beta, g)
        r = tc.check_reg(h, alpha, beta, 1.0 if g is None else g, mode, got['out3'], got['dh'], ctx)
        _say('RATIO %-34s %s' % (ctx, tc.fmt_ratios(r)))
        assert max(r.values()) <= 1.0
        if case.T == 1:
            ref = tc.reg_reference(h, alpha, 0.0, 1.0 if g is None else g)                   # no TAR gradient at all
            assert tc._ratio(got['dh'].ravel(), ref['dh'].ravel(), ref['dh_bound'].ravel(), 'dh at T = 1', ctx) <= 1.0


def test_seq_reg_workspace_one_byte_short():
    check, lib, ptr, stream = _abi()
    h = _dev(tc.reg_data(tc.REG_CASES[2], 'randn'))
    T, R = h.shape
    wsb = int(lib.nnl_seq_reg_workspace_bytes(T, R))
    ws, out3 = Band(wsb // 4), Band(3)
    assert lib.nnl_seq_reg_fwd(ptr(h), ptr(out3.view), T, R, 2.0, 1.0, ptr(ws.view), wsb - 1, stream()) == -4        # NNL_ERR_WORKSPACE
    assert b'seq_reg_fwd' in lib.nnl_last_error()
    assert lib.nnl_seq_reg_fwd(ptr(h), ptr(out3.view), T, R, 2.0, 1.0, None, wsb, stream()) == -4
    torch.cuda.synchronize()
    assert np.isnan(out3.get('out3', 'short workspace')).all() and np.isnan(ws.get('workspace', 'short workspace')).all(), 'something ran'


# ---- weight drop ------------------------------------------------------------------------------------------------------------------------------
def run_wd(c, src, mask, ctx):
    check, lib, ptr, stream = _abi()
    ld_out = tc.wd_ld_out(c.H, c.ld_out)
    d_src, d_mask = _dev(src), _dev(mask)
    out = Band(c.rows * ld_out)
    check(lib.nnl_weight_drop(ptr(d_src), c.ld_src, ptr(d_mask), ptr(out.view), ld_out, c.rows, c.H, c.seed, c.p, stream()))
    torch.cuda.synchronize()
    _unchanged(d_src, src, 'src', ctx)
    _unchanged(d_mask, mask, 'mask', ctx)
    return dict(out=out.get('out', ctx).reshape(c.rows, ld_out))


@pytest.mark.parametrize('case', tc.WD_CASES, ids=tc.case_id)
def test_weight_drop(case):
    src, mask = tc.wd_data(case)
    got = _twice(run_wd, 'wd-' + case.name, case, src, mask)
    keep = tc.check_wd(case, src, mask, got['out'], 'wd-' + case.name)
    if keep is None:
        _say('RATIO wd %-10s bit for bit' % case.name)
        return
    sig = tc.wd_share_sigmas(keep, case.p)
    _say('RATIO wd %-10s bit for bit; kept %.4f of %d (p = %g): %.2f sigma' % (case.name, keep.mean(), keep.size, case.p, sig))
    assert sig < 5.0
    scale = got['out'][:, :case.H][keep] / src[:, :case.H][keep]
    assert np.allclose(scale[np.isfinite(scale)], tc.wd_scale(case.p), rtol=2e-7)


@pytest.mark.parametrize('p', tc.WD_P)
@pytest.mark.parametrize('seed', tc.WD_SEEDS)
def test_weight_drop_forward_and_backward_share_the_mask(seed, p):
    "W = raw * m into rows padded to 32, then dW_raw = dW * m out of a padded dW (ld_out = H): the same elements survive"
    rows, H, Hp = 24, 115, 128
    r = np.random.RandomState(7)
    raw = (r.rand(rows, H) + 0.5).astype(F32)
    dwp = np.zeros((rows, Hp), dtype=F32)
    dwp[:, :H] = r.rand(rows, H) + 0.5
    fwd = tc.WDCase('f', rows, H, H, 'ceil32', 'hash', p, seed, [])
    bwd = tc.WDCase('b', rows, H, Hp, 'H', 'hash', p, seed, [])
    w = _twice(run_wd, 'wd-fwd', fwd, raw, None)['out']
    dw = _twice(run_wd, 'wd-bwd', bwd, dwp, None)['out']
    keep = tc.check_wd(fwd, raw, None, w, 'wd-fwd seed %x p %g' % (seed, p))
    assert np.array_equal(tc.check_wd(bwd, dwp, None, dw, 'wd-bwd seed %x p %g' % (seed, p)), keep)
    assert np.array_equal(w[:, :H] != 0, keep) and np.array_equal(dw != 0, keep)
    _say('RATIO wd seed %x p %g: forward and backward keep the same %d of %d' % (seed, p, keep.sum(), keep.size))


# ---- argument checks: refused before any launch ---------------------------------------------------------------------------------------------------
def test_bad_arguments():
    check, lib, ptr, stream = _abi()
    f, i = Band(64), Band(8, torch.int64, fill=0)
    p, q, s = ptr(f.view), ptr(i.view), stream()
    ws = Band(2048)
    calls = [
        ('softmax_ce_fwd', lambda: lib.nnl_softmax_ce_fwd(None, q, p, p, p, 2, 4, None, s)),
        ('softmax_ce_fwd', lambda: lib.nnl_softmax_ce_fwd(p, q, None, p, p, 2, 4, None, s)),
        ('softmax_ce_fwd', lambda: lib.nnl_softmax_ce_fwd(p, q, p, p, p, 0, 4, None, s)),
        ('softmax_ce_fwd', lambda: lib.nnl_softmax_ce_fwd(p, q, p, p, p, 2, 0, None, s)),
        ('softmax_ce_bwd', lambda: lib.nnl_softmax_ce_bwd(p, q, p, p, None, 2, 4, 4, s)),
        ('softmax_ce_bwd', lambda: lib.nnl_softmax_ce_bwd(p, q, p, None, p, 2, 4, 4, s)),
        ('softmax_ce_bwd', lambda: lib.nnl_softmax_ce_bwd(p, q, p, p, p, 0, 4, 4, s)),
        ('softmax_ce_bwd', lambda: lib.nnl_softmax_ce_bwd(p, q, p, p, p, 2, 4, 3, s)),                  # ld_dlogits < V
        ('embedding_rowmask_fwd', lambda: lib.nnl_embedding_rowmask_fwd(None, p, None, p, 2, 4, 4, None, s)),
        ('embedding_rowmask_fwd', lambda: lib.nnl_embedding_rowmask_fwd(q, p, None, p, 2, 0, 4, None, s)),
        ('embedding_rowmask_bwd', lambda: lib.nnl_embedding_rowmask_bwd(q, None, p, None, 2, 4, 4, -1, None, 0, s)),
        ('embedding_rowmask_bwd', lambda: lib.nnl_embedding_rowmask_bwd(q, None, p, p, 2, 4, 0, -1, None, 0, s)),
        ('seq_reg_fwd', lambda: lib.nnl_seq_reg_fwd(None, p, 2, 4, 2.0, 1.0, ptr(ws.view), 8192, s)),
        ('seq_reg_fwd', lambda: lib.nnl_seq_reg_fwd(p, p, 0, 4, 2.0, 1.0, ptr(ws.view), 8192, s)),
        ('seq_reg_bwd', lambda: lib.nnl_seq_reg_bwd(p, None, None, 2, 4, 2.0, 1.0, s)),
        ('seq_reg_bwd', lambda: lib.nnl_seq_reg_bwd(p, None, p, 2, 0, 2.0, 1.0, s)),
        ('weight_drop', lambda: lib.nnl_weight_drop(None, 4, None, p, 4, 2, 4, 0, 0.5, s)),
        ('weight_drop', lambda: lib.nnl_weight_drop(p, 4, None, p, 4, 0, 4, 0, 0.5, s)),
        ('weight_drop', lambda: lib.nnl_weight_drop(p, 4, None, p, 4, 2, 4, 0, 1.0, s)),                # p = 1
        ('weight_drop', lambda: lib.nnl_weight_drop(p, 4, None, p, 4, 2, 4, 0, -0.1, s)),
        ('weight_drop', lambda: lib.nnl_weight_drop(p, 3, None, p, 4, 2, 4, 0, 0.5, s)),                # ld_src < H
        ('weight_drop', lambda: lib.nnl_weight_drop(p, 4, None, p, 3, 2, 4, 0, 0.5, s)),                # ld_out < H
    ]
    for k, (name, call) in enumerate(calls):
        (st, notes) = _notes(lib, call)
        assert st == -1 and name.encode() in lib.nnl_last_error(), 'call %d (%s): status %d, "%s"' % (k, name, st, lib.nnl_last_error().decode())
        assert notes == []
    torch.cuda.synchronize()
    assert np.isnan(f.get('the float operand', 'bad arguments')).all() and not i.get('the index operand', 'bad arguments').any()
    assert np.isnan(ws.get('the workspace', 'bad arguments')).all()


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------------
def _ce_nd_reference(preds_cpu, target_cpu, gout):
    p = preds_cpu.detach().double().requires_grad_()
    loss = F.cross_entropy(p, target_cpu)
    loss.backward(torch.tensor(gout, dtype=torch.float64))
    return loss.detach(), p.grad


@pytest.mark.parametrize('shape', [(7, 10), (5, 10, 3), (3, 37, 4, 2)], ids=['N,C', 'N,C,d1', 'N,C,d1,d2'])
def test_cross_entropy_nd_contiguous(shape):
    from neuralnetworklibrary_amd import ops
    g = torch.Generator().manual_seed(len(shape))
    preds = 3 * torch.randn(*shape, generator=g)
    target = torch.randint(0, shape[1], (shape[0],) + shape[2:], generator=g)
    want, want_grad = _ce_nd_reference(preds, target, 2.5)
    p = preds.to(DEV).requires_grad_()
    loss = ops.cross_entropy_nd(p, target.to(DEV))
    loss.backward(torch.tensor(2.5, device=DEV))
    assert_close(loss, want, 2e-6, 1e-7, 'cross_entropy_nd %s' % (shape,))
    assert p.grad.shape == p.shape and p.grad.stride() == p.stride(), 'the gradient is not in the input\'s layout'
    assert_close(p.grad, want_grad, 1e-5, 1e-8, 'gradient of cross_entropy_nd %s' % (shape,))


def test_cross_entropy_nd_permuted_view_of_the_decoder_buffer():
    "[bs, V, seq] as the permute(1, 2, 0) view of a contiguous [seq, bs, V] buffer: used as is, the gradient arrives in that buffer"
    from neuralnetworklibrary_amd import ops
    seq, bs, V = 6, 3, 37
    g = torch.Generator().manual_seed(5)
    buf = 3 * torch.randn(seq, bs, V, generator=g)
    target = torch.randint(0, V, (bs, seq), generator=g)
    want, want_grad = _ce_nd_reference(buf.permute(1, 2, 0), target, 1.0)
    b = buf.to(DEV).requires_grad_()
    view = b.permute(1, 2, 0)
    assert view.permute(2, 0, 1).is_contiguous() and not view.is_contiguous()
    loss = ops.cross_entropy_nd(view, target.to(DEV))
    loss.backward()
    assert_close(loss, want, 2e-6, 1e-7, 'cross_entropy_nd on the permuted view')
    assert b.grad.shape == b.shape and b.grad.is_contiguous()
    assert_close(b.grad.permute(1, 2, 0), want_grad, 1e-5, 1e-8, 'gradient on the permuted view')


def test_padded_gradient_hand_over():
    """V = 10: the backward writes into rows of 16 floats with zeros behind column 10 and registers the buffer, so that the backward of the
    linear layer that produced the logits runs on it as it is"""
    from neuralnetworklibrary_amd import ops
    rows, V, K = 9, 10, 12
    g = torch.Generator().manual_seed(11)
    x, w, b = torch.randn(rows, K, generator=g), torch.randn(V, K, generator=g), torch.randn(V, generator=g)
    target = torch.randint(0, V, (rows,), generator=g)
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    F.cross_entropy(F.linear(xr, wr, br), target).backward()
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, b))
    logits = ops.linear(xd, wd, bd)
    seen = {}

    def hook(grad):
        base = grad._base
        seen.update(view=grad._is_view(), base_shape=None if base is None else tuple(base.shape), stride=grad.stride(),
                    ld=None if base is None else ops._PADDED_GRADS.get(id(base), (None, None))[1],
                    pad=None if base is None else base[:, V:].abs().max().item())

    logits.register_hook(hook)
    ops.softmax_cross_entropy(logits, target.to(DEV)).backward()
    assert seen == dict(view=True, base_shape=(rows, 16), stride=(16, 1), ld=16, pad=0.0), seen
    for got, want, what in ((xd.grad, xr.grad, 'dx'), (wd.grad, wr.grad, 'dW'), (bd.grad, br.grad, 'db')):
        assert_close(got, want, 2e-5, 2e-6, 'padded hand-over: ' + what)
