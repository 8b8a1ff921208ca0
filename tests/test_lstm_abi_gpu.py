"""The LSTM C ABI (nnl_lstm_fwd / nnl_lstm_bwd; include/nnl.h) called directly, route by route, over the cases of tests/lstm_cases.py,
against their fp64 reference — without the GEMMs and the weight drop that ops_text.lstm_layer wraps around the recurrence.

Per case: the switches are set and nnl_reload_env() called; the route note of each call must name the kernel, template arguments and
plan the case expects (a cooperative launch that was refused shows as the fallback's note and fails the test); the workspace has
exactly nnl_lstm_workspace_bytes bytes, sits between guard bands and is filled with 0xFF bytes before every call (in the product it is
a shared scratch buffer with other operators' leftovers: the library zeroes what it needs); outputs are pre-filled with a sentinel,
dgates_pad with zero in its pad columns; the backward gets the fp64 reference's gates and cy rounded to fp32, so that each backward
route is judged on its own; err_flag must read 0; a second run on the same inputs must be bitwise equal.  One more test chains the
library's forward into its backward, one case per backward route.  No test provokes a barrier time-out.

The file takes about 2 s on an MI355X (45 tests in 1.65 s, the slowest case 0.3 s, most under 0.1 s).
"""
import ctypes
import os
import sys

import pytest
import torch

import lstm_cases as lc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                                     # bytes (workspace) or elements (outputs) of guard band on either side of a buffer
SWITCHES = ('NNL_LSTM_PERSIST', 'NNL_LSTM_FUSED_BWD')
IDX = list(range(len(lc.CASES)))
ids = lambda i: lc.case_id(lc.CASES[i])


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


@pytest.fixture
def lstm_switches():
    """sets the two switches for a case; afterwards restores the variables and makes the library read them again, so that its cached
    values never outlive the test"""
    from neuralnetworklibrary_amd._lib import lib
    saved = {k: os.environ.get(k) for k in SWITCHES}

    def set_(case):
        os.environ['NNL_LSTM_PERSIST'] = str(case.persist)
        os.environ['NNL_LSTM_FUSED_BWD'] = str(case.fused)
        lib.nnl_reload_env()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    lib.nnl_reload_env()


class Guarded:
    """`numel` float32 elements (or bytes) inside a larger allocation with guard bands on both sides"""

    def __init__(self, numel, dtype=torch.float32):
        self.numel = numel
        self.band = 0xA5 if dtype == torch.uint8 else -54321.0
        self.buf = torch.full((numel + 2 * GUARD,), self.band, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + numel]

    def intact(self):
        return bool((self.buf[:GUARD] == self.band).all()) and bool((self.buf[GUARD + self.numel:] == self.band).all())


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def plan_of(lib, c):
    out = (ctypes.c_int32 * 14)()
    assert lib.nnl_debug_lstm_plan(c.B, c.H, out) == 1
    return lc.Plan(*out)


def lstm_notes(lib, call):
    """(status, the lstm_* route notes of the call)"""
    buf = ctypes.create_string_buffer(16384)
    lib.nnl_debug_route_record(1)
    try:
        st = call()
        assert lib.nnl_debug_route_collect(buf, len(buf)) >= 0
    finally:
        lib.nnl_debug_route_record(0)
    return st, [n for n in buf.value.decode().split(';') if n.startswith('lstm_')]


class Harness:
    """device operands of one case and the two calls"""

    def __init__(self, lib, c):
        self.lib, self.c = lib, c
        self.p = p = plan_of(lib, c)
        T, B, H = c.T, c.B, c.H
        d = lc.make_inputs(c)
        self.x = {k: (None if v is None else v.to(DEV)) for k, v in d.items()}
        w = self.x['w_hh']
        self.w_pad = torch.nn.functional.pad(w, (0, p.Hp - H)).contiguous()                     # [4H, Hp]
        self.w_t_pad = torch.nn.functional.pad(w.t().contiguous(), (0, p.Gp - 4 * H)).contiguous()   # [H, Gp]
        self.wsb = int(lib.nnl_lstm_workspace_bytes(T, B, H))
        assert self.wsb > 0 and self.wsb % 4 == 0
        self.ws = Guarded(self.wsb, torch.uint8)
        assert self.ws.t.data_ptr() % 8 == 0
        self.err = None if 'err_flag' in c.nulls else torch.zeros(1, dtype=torch.int32, device=DEV)
        self.notes = lc.route_notes(c, p)

    def _out(self, *shape):
        n = 1
        for s in shape:
            n *= s
        g = Guarded(n)
        g.t.fill_(lc.SENTINEL)
        return g, g.t.view(*shape)

    def forward(self):
        c, lib, x = self.c, self.lib, self.x
        T, B, H = c.T, c.B, c.H
        bufs = {}
        bufs['y'], y = self._out(T, B, H)
        bufs['cy'], cy = self._out(T, B, H)
        bufs['gates'], gates = self._out(T, B, 4 * H)
        self.ws.t.fill_(0xFF)
        st, notes = lstm_notes(lib, lambda: lib.nnl_lstm_fwd(ptr(x['gx']), ptr(self.w_pad), ptr(x['h0']), ptr(x['c0']), ptr(y), ptr(cy), ptr(gates),
                                                             T, B, H, ptr(self.ws.t), self.wsb, ptr(self.err), None))
        torch.cuda.synchronize()
        assert st == 0, 'nnl_lstm_fwd: %d %s' % (st, lib.nnl_last_error())
        assert notes == [self.notes[0]], '%s: forward took %s, the case is there for %s' % (lc.case_id(c), notes, self.notes[0])
        self._after(bufs, 'nnl_lstm_fwd')
        return dict(y=y, cy=cy, gates=gates)

    def backward(self, gates, cy):
        c, lib, x, p = self.c, self.lib, self.x, self.p
        T, B, H = c.T, c.B, c.H
        bufs = {}
        bufs['dgates_pad'], tape = self._out(T, B, p.Gp)
        tape[..., 4 * H:] = 0.0                                                        # the header: pad columns zero on entry
        bufs['dh0'], dh0 = self._out(B, H)
        bufs['dc0'], dc0 = self._out(B, H)
        self.ws.t.fill_(0xFF)
        st, notes = lstm_notes(lib, lambda: lib.nnl_lstm_bwd(ptr(x['dy']), ptr(x['dhT']), ptr(x['dcT']), ptr(gates), ptr(cy), ptr(x['c0']),
                                                             ptr(self.w_t_pad), ptr(tape), ptr(dh0), ptr(dc0), T, B, H, ptr(self.ws.t),
                                                             self.wsb, ptr(self.err), None))
        torch.cuda.synchronize()
        assert st == 0, 'nnl_lstm_bwd: %d %s' % (st, lib.nnl_last_error())
        assert notes == [self.notes[1]], '%s: backward took %s, the case is there for %s' % (lc.case_id(c), notes, self.notes[1])
        self._after(bufs, 'nnl_lstm_bwd')
        return dict(dgates_pad=tape, dh0=dh0, dc0=dc0)

    def _after(self, bufs, what):
        ctx = '%s: %s' % (lc.case_id(self.c), what)
        for name, g in bufs.items():
            assert g.intact(), '%s wrote outside %s (guard band touched)' % (ctx, name)
        assert self.ws.intact(), '%s wrote outside its workspace of %d bytes' % (ctx, self.wsb)
        if self.err is not None:
            assert int(self.err.item()) == 0, '%s: err_flag reads %d' % (ctx, int(self.err.item()))


def _bitwise(a, b, ctx):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), '%s: %s differs between two runs on the same inputs' % (ctx, k)


def _check(out, ref, c, route):
    cpu = {k: v.cpu() for k, v in out.items()}
    rep = lc.check(cpu, ref, c, cpu32=lambda: lc.recurrence(c, torch.float32))
    for name, (ratio, err, e32) in rep.items():
        _say('LSTM_ABI %s %s %s worst %.3f of the tolerance, max abs err %.3e%s' % (
            lc.case_id(c), route, name, ratio, err, '' if e32 is None else ' (fp32 on the CPU: %.3e)' % e32))


@pytest.mark.parametrize('i', IDX, ids=ids)
def test_lstm_abi_route_by_route_vs_fp64(i, lstm_switches):
    from neuralnetworklibrary_amd._lib import lib
    c, ref = lc.CASES[i], lc.reference(i)
    lstm_switches(c)
    h = Harness(lib, c)
    fwd = h.forward()
    _check(fwd, ref, c, h.notes[0])
    _bitwise(fwd, h.forward(), lc.case_id(c) + ' forward')
    gates, cy = ref['gates'].float().to(DEV), ref['cy'].float().to(DEV)
    bwd = h.backward(gates, cy)
    _check(bwd, ref, c, h.notes[1])
    _bitwise(bwd, h.backward(gates, cy), lc.case_id(c) + ' backward')
    assert torch.equal(gates, ref['gates'].float().to(DEV)) and torch.equal(cy, ref['cy'].float().to(DEV)), 'the backward wrote to its inputs'


@pytest.mark.parametrize('c', lc.CHAINED, ids=lc.case_id)
def test_lstm_abi_forward_chained_into_backward(c, lstm_switches):
    """as the product calls them: the backward reads the gates and cy the library's own forward saved"""
    from neuralnetworklibrary_amd._lib import lib
    ref = lc.reference(lc.CASES.index(c))
    lstm_switches(c)
    h = Harness(lib, c)
    fwd = h.forward()
    bwd = h.backward(fwd['gates'], fwd['cy'])
    _check(bwd, ref, c, h.notes[0] + ' -> ' + h.notes[1])


def test_default_switches_take_the_persistent_forward_and_the_2d_bptt(lstm_switches):
    """with neither switch in the environment (the fixture puts back whatever was there) a call takes the default routes: what a
    switch test that ran before may have left cached in the library does not count"""
    from neuralnetworklibrary_amd._lib import lib
    for k in SWITCHES:
        os.environ.pop(k, None)
    lib.nnl_reload_env()
    c = lc.C(2, 4, 37, 'persist', 'bptt2', 5, [])
    ref = lc.recurrence(c, torch.float64)
    h = Harness(lib, c)
    assert h.notes == ('lstm_persist_fwd<1>@37', 'lstm_bptt2<1,16>@10x3')
    _check(h.forward(), ref, c, h.notes[0])
    _check(h.backward(ref['gates'].float().to(DEV), ref['cy'].float().to(DEV)), ref, c, h.notes[1])
