"""The detection-loss C ABI (nnl_retina_loss_fwd / nnl_retina_loss_bwd; K6 in include/nnl.h) called directly over the cases of
tests/retina_cases.py, against their reference — without ops.retina_loss around it.

Per case: the workspace has exactly nnl_retina_loss_workspace_bytes bytes, sits between guard bands and is filled with 0xFF bytes before
every call; state, npos, out, dreg and dclas sit between guard bands and are pre-filled with a sentinel: afterwards the bands are intact
and no sentinel is left inside (at A = 9 and A = 257 that is the tail chunk: every element written, nothing past it).  The forward's
state and npos must EQUAL the fp32 restatement of the matching, out must sit within 2e-5 of fp64.  The backward gets the reference's state
and npos, so that it is judged on its own: per-element tolerances, exact zeros off the positives / on ignored anchors / outside the clamp
range, nonzero on the range's two ends (retina_cases.check_backward).  A second run of either call is bitwise equal.  Then: the kernel's own
state chained into its backward, one case per class path; padding rows moved among the valid rows change no bit; an image alone gives
what it gives inside a batch of 17.  All indices and categories are valid: no test provokes a fault.

The file takes about 1.2 s on an MI355X (30 tests in 1.15 s; the slowest is the first case at 0.36 s, which loads the library and
initialises the device, then k4-a16385 at 0.09 s; every other test 0.02 s or less).
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import retina_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 4096                                     # elements (bytes for the workspace) of guard band on either side of a buffer
BANDS = {torch.uint8: 0xA5, torch.int32: 0x3C3C3C3C, torch.float32: -54321.0}
IDX = list(range(len(rc.CASES)))
ids = lambda i: rc.CASES[i].name


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


class Guarded:
    """`numel` elements inside a larger allocation with guard bands on both sides, pre-filled with `fill`"""

    def __init__(self, numel, dtype, fill):
        self.numel, self.band, self.fill = numel, BANDS[dtype], fill
        self.buf = torch.full((numel + 2 * GUARD,), self.band, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + numel]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[:GUARD] == self.band).all()) and bool((self.buf[GUARD + self.numel:] == self.band).all())

    def unwritten(self):
        return int((self.t == self.fill).sum())


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Harness:
    """device operands of one case (or of `inputs` with the case's hyper-parameters) and the two calls"""

    def __init__(self, lib, c, inputs=None):
        self.lib, self.c = lib, c
        d = rc.make_inputs(c) if inputs is None else inputs
        self.bs, self.A, self.K = d['clas'].shape
        self.M = d['cats'].shape[1]
        self.host = d
        self.x = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in d.items()}
        if self.M == 0:                                                  # the header: M = 0 may come with NULL
            self.x['boxes'] = self.x['cats'] = None
        else:
            assert ((d['cats'] == -1) | ((d['cats'] >= 0) & (d['cats'] < self.K))).all(), 'a test never passes an invalid category'
        self.gup = torch.tensor([c.g], dtype=torch.float32, device=DEV)
        self.wsb = int(lib.nnl_retina_loss_workspace_bytes(self.bs, self.A))
        assert self.wsb == self.bs * rc.cdiv(self.A, 256) * 12
        self.ws = Guarded(self.wsb, torch.uint8, 0xFF)
        self.name = '%s [bs %d, A %d, K %d, M %d]' % (c.name, self.bs, self.A, self.K, self.M)

    def _after(self, bufs, what):
        for name, g in bufs.items():
            assert g.intact(), '%s: %s wrote outside %s (guard band touched)' % (self.name, what, name)
            assert g.unwritten() == 0, '%s: %s left %d of %d elements of %s unwritten' % (self.name, what, g.unwritten(), g.numel, name)
        assert self.ws.intact(), '%s: %s wrote outside its workspace of %d bytes' % (self.name, what, self.wsb)
        for k, v in self.host.items():
            if self.x[k] is not None:
                assert torch.equal(self.x[k].cpu(), torch.from_numpy(np.array(v))), '%s: %s wrote to its input %s' % (self.name, what, k)

    def forward(self):
        c, lib, x = self.c, self.lib, self.x
        bufs = dict(state=Guarded(self.bs * self.A, torch.int32, rc.STATE_SENTINEL), npos=Guarded(self.bs, torch.float32, rc.SENTINEL),
                    out=Guarded(3, torch.float32, rc.SENTINEL))
        self.ws.t.fill_(0xFF)
        st = lib.nnl_retina_loss_fwd(ptr(x['anchors']), ptr(x['reg']), ptr(x['clas']), ptr(x['boxes']), ptr(x['cats']), ptr(bufs['state'].t),
                                     ptr(bufs['npos'].t), ptr(bufs['out'].t), self.bs, self.A, self.K, self.M, c.beta, c.alpha, c.gamma,
                                     ptr(self.ws.t), self.wsb, None)
        torch.cuda.synchronize()
        assert st == 0, 'nnl_retina_loss_fwd: %d %s' % (st, lib.nnl_last_error())
        self._after(bufs, 'nnl_retina_loss_fwd')
        return dict(state=bufs['state'].t.view(self.bs, self.A).cpu().numpy(), npos=bufs['npos'].t.cpu().numpy(), out=bufs['out'].t.cpu().numpy())

    def backward(self, state, npos):
        c, lib, x = self.c, self.lib, self.x
        st_d = torch.from_numpy(np.ascontiguousarray(state, np.int32)).to(DEV)
        np_d = torch.from_numpy(np.ascontiguousarray(npos, np.float32)).to(DEV)
        bufs = dict(dreg=Guarded(self.bs * self.A * 4, torch.float32, rc.SENTINEL), dclas=Guarded(self.bs * self.A * self.K, torch.float32, rc.SENTINEL))
        st = lib.nnl_retina_loss_bwd(ptr(x['anchors']), ptr(x['reg']), ptr(x['clas']), ptr(x['boxes']), ptr(x['cats']), ptr(st_d), ptr(np_d),
                                     ptr(self.gup), ptr(bufs['dreg'].t), ptr(bufs['dclas'].t), self.bs, self.A, self.K, self.M, c.beta, c.alpha,
                                     c.gamma, None)
        torch.cuda.synchronize()
        assert st == 0, 'nnl_retina_loss_bwd: %d %s' % (st, lib.nnl_last_error())
        self._after(bufs, 'nnl_retina_loss_bwd')
        assert np.array_equal(st_d.cpu().numpy(), np.asarray(state, np.int32)) and np.array_equal(np_d.cpu().numpy(), np.asarray(npos, np.float32))
        return dict(dreg=bufs['dreg'].t.view(self.bs, self.A, 4).cpu().numpy(), dclas=bufs['dclas'].t.view(self.bs, self.A, self.K).cpu().numpy())


def _bitwise(a, b, ctx):
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), '%s: %s differs' % (ctx, k)


@pytest.mark.parametrize('i', IDX, ids=ids)
def test_retina_abi_case_by_case_vs_fp64(i):
    from neuralnetworklibrary_amd._lib import lib
    c = rc.CASES[i]
    r = rc.reference(c)
    h = Harness(lib, c)
    fwd = h.forward()
    _say('RETINA_ABI %s out %s fp64 %s' % (c.name, fwd['out'], r['out']))
    q_out = rc.check_forward(c, r, fwd['state'], fwd['npos'], fwd['out'])
    _bitwise(fwd, h.forward(), c.name + ' forward, two runs on the same inputs')
    bwd = h.backward(r['state'], r['npos'])
    e_r, e_c = np.abs(bwd['dreg'] - r['dreg']).max(), np.abs(bwd['dclas'] - r['dclas']).max()
    _say('RETINA_ABI %s max abs err dreg %.3e dclas %.3e' % (c.name, e_r, e_c))
    q_reg, q_clas = rc.check_backward(c, r, bwd['dreg'], bwd['dclas'])
    _say('RETINA_ABI %s err / tolerance: out %.3f dreg %.3f dclas %.3f' % (c.name, q_out, q_reg, q_clas))
    _bitwise(bwd, h.backward(r['state'], r['npos']), c.name + ' backward, two runs on the same inputs')


@pytest.mark.parametrize('name', rc.CHAINED)
def test_retina_abi_forward_chained_into_backward(name):
    """as the product calls them: the backward reads the state and npos the library's own forward saved"""
    from neuralnetworklibrary_amd._lib import lib
    c = rc.case(name)
    r = rc.reference(c)
    h = Harness(lib, c)
    fwd = h.forward()
    rc.check_forward(c, r, fwd['state'], fwd['npos'], fwd['out'])
    bwd = h.backward(fwd['state'], fwd['npos'])
    q_reg, q_clas = rc.check_backward(c, r, bwd['dreg'], bwd['dclas'], ' (chained)')
    _say('RETINA_ABI %s chained err / tolerance: dreg %.3f dclas %.3f' % (c.name, q_reg, q_clas))


def test_moving_the_padding_rows_changes_no_bit():
    """the padding rows of every image moved behind its valid rows, whose order is kept: the compacted object list is the same, so is
    every output, bit for bit"""
    from neuralnetworklibrary_amd._lib import lib
    c = rc.case(rc.PERMUTED)
    d = dict(rc.make_inputs(c))
    moved = dict(d)
    moved['boxes'], moved['cats'] = rc.pad_to_end(d['boxes'], d['cats'])
    assert not np.array_equal(moved['cats'], d['cats']) and all((moved['cats'][i] >= 0).sum() == (d['cats'][i] >= 0).sum() for i in range(c.bs))
    h1, h2 = Harness(lib, c), Harness(lib, c, moved)
    f1, f2 = h1.forward(), h2.forward()
    _bitwise(f1, f2, c.name + ' forward, padding between the valid rows vs at the end')
    _bitwise(h1.backward(f1['state'], f1['npos']), h2.backward(f2['state'], f2['npos']), c.name + ' backward, padding between the valid rows vs at the end')
    rc.check_forward(c, rc.reference(c), f2['state'], f2['npos'], f2['out'])


def test_an_image_alone_gives_what_it_gives_inside_the_batch():
    """batch of 17 (wave 0 of the finalize owns images 0 and 16): image i alone has the same state and npos, its two terms sit within the
    forward tolerance of the fp64 per-image terms, and their means are the batch's out"""
    from neuralnetworklibrary_amd._lib import lib
    c = rc.case(rc.ALONE)
    d, r = rc.make_inputs(c), rc.reference(c)
    batch = Harness(lib, c).forward()
    rc.check_forward(c, r, batch['state'], batch['npos'], batch['out'])
    terms = np.zeros((c.bs, 2))
    for i in range(c.bs):
        one = {k: (v if k == 'anchors' else v[i:i + 1]) for k, v in d.items()}
        f = Harness(lib, c, one).forward()
        assert np.array_equal(f['state'][0], batch['state'][i]) and f['npos'][0] == batch['npos'][i], 'image %d' % i
        want = np.array([r['img_reg'][i], r['img_clas'][i]])
        assert (np.abs(f['out'][1:].astype(np.float64) - want) <= rc.OUT_RTOL * np.abs(want)).all(), 'image %d alone: %s, fp64 %s' % (i, f['out'][1:], want)
        terms[i] = f['out'][1:]
    mean = terms.mean(0)
    assert (np.abs(batch['out'][1:].astype(np.float64) - mean) <= rc.OUT_RTOL * np.abs(mean)).all(), 'batch %s, mean of the images alone %s' % (batch['out'][1:], mean)
