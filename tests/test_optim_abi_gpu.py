"""The optimizer-step C ABI (nnl_optim_step, nnl_optim_patch; include/nnl.h) called directly over the launch regimes of csrc/optim.hip,
against the fp64 reference of tests/optim_cases.py, and the host class on top of it (fused_optim.FusedStep through General.Optimizer)
against the reference semantics in fp64 on the CPU.

Every case of optim_cases.CASES runs as SGD and as Adam, in both data modes (`dyadic`: bit for bit; `randn`: derived elementwise
bounds, see optim_cases) and with the clip off, active and inactive.  Around every call: parameters, gradients and states sit in one
allocation each, three sentinel floats between neighbouring tensors and a band on either side, the memory of a NULL gradient included;
the workspace has exactly the documented n_chunks + 2 floats between bands; the call is repeated from the same state and must reproduce
itself bit for bit.  Every test prints max err / bound.
"""
import copy
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_cases as oc
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GAP, GUARD = 3, 1024                             # sentinel floats between two tensors / on either side of an allocation
SENT = np.float32(12345.0)


def _say(*a):
    print(*a, flush=True)
    sys.stdout.flush()


class Arena:
    """where the tensors of a case lie inside one allocation: GUARD sentinels, tensor 0, GAP sentinels, tensor 1, ..., GUARD sentinels"""

    def __init__(self, sizes):
        self.starts, o = [], GUARD
        for n in sizes:
            self.starts.append(o)
            o += n + GAP
        self.total = o - GAP + GUARD
        self.pos = np.concatenate([np.arange(s, s + n) for s, n in zip(self.starts, sizes)])
        self.outside = np.ones(self.total, dtype=bool)
        self.outside[self.pos] = False

    def upload(self, flat):
        host = np.full(self.total, SENT, dtype=np.float32)
        host[self.pos] = flat
        return torch.from_numpy(host).to(DEV)

    def download(self, buf, what, ctx):
        a = buf.cpu().numpy()
        assert np.array_equal(oc.bits(a[self.outside]), oc.bits(np.full(int(self.outside.sum()), SENT))), \
            '%s: wrote outside a tensor of %s (sentinel touched)' % (ctx, what)
        return a[self.pos]


def run_step(data, hyper, clip, ctx):
    """one nnl_optim_step from the state in `data`; returns dict(p, g, s1, s2, norm, coef) as numpy fp32"""
    from neuralnetworklibrary_amd._lib import check, lib, ptr, stream
    desc = data['desc'].copy()
    arena = Arena([int(n) for n in desc['numel']])
    bufs = {k: arena.upload(data[k]) for k in ('p', 'g', 's1', 's2')}
    for t, s in enumerate(arena.starts):
        desc['param'][t] = bufs['p'].data_ptr() + 4 * s
        desc['grad'][t] = 0 if data['desc']['grad'][t] == 0 else bufs['g'].data_ptr() + 4 * s
        desc['s1'][t] = bufs['s1'].data_ptr() + 4 * s
        desc['s2'][t] = bufs['s2'].data_ptr() + 4 * s
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    d_ct, d_co = torch.from_numpy(data['chunk_tensor']).to(DEV), torch.from_numpy(data['chunk_off']).to(DEV)
    d_hyper = torch.from_numpy(np.asarray(hyper, dtype=np.float32)).to(DEV)
    n_chunks = len(data['chunk_tensor'])
    use_clip = clip != 'off'
    ws = None
    if use_clip:
        ws = torch.full((n_chunks + 2 + 2 * GUARD,), float(SENT), dtype=torch.float32, device=DEV)
        ws[GUARD:GUARD + n_chunks + 2] = float('nan')
    check(lib.nnl_optim_step(ptr(d_desc), ptr(d_ct), ptr(d_co), n_chunks, data['kind'], ptr(d_hyper), 1 if use_clip else 0,
                             None if ws is None else ptr(ws[GUARD:]), stream()))
    torch.cuda.synchronize()
    got = {k: arena.download(bufs[k], k, ctx) for k in bufs}
    got.update(norm=None, coef=None)
    if use_clip:
        w = ws.cpu().numpy()
        assert (w[:GUARD] == SENT).all() and (w[GUARD + n_chunks + 2:] == SENT).all(), '%s: wrote outside the clip workspace' % ctx
        got.update(coef=w[GUARD], norm=w[GUARD + 1], partial=w[GUARD + 2:GUARD + 2 + n_chunks].copy())
    assert np.array_equal(d_desc.cpu().numpy(), desc.view(np.uint8)) and np.array_equal(d_hyper.cpu().numpy(), np.asarray(hyper, dtype=np.float32))
    return got


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(oc.bits(a[k]), oc.bits(b[k])) for k in a)


def run_twice(data, hyper, clip, ctx):
    a = run_step(data, hyper, clip, ctx)
    b = run_step(data, hyper, clip, ctx)
    assert _same(a, b), '%s: two calls from the same state differ (not bitwise reproducible)' % ctx
    return a


# ---- nnl_optim_step over the launch regimes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', oc.MODES)
@pytest.mark.parametrize('kind,kname', oc.KINDS, ids=[k[1] for k in oc.KINDS])
@pytest.mark.parametrize('case', oc.CASES, ids=oc.case_id)
def test_sweep(case, kind, kname, mode):
    data = oc.make_data(case, kind, mode)
    off = None
    for clip in case.clips:
        ctx = '%s-%s-%s-clip %s' % (case.name, kname, mode, clip)
        hyper = oc.hyper_of(kind, mode, case.momentum, data['t'], oc.max_norm_of(data, clip))
        got = run_twice(data, hyper, clip, ctx)
        if clip != 'off':
            assert not np.isnan(got['partial']).any(), '%s: a partial sum of the norm was never written' % ctx
        r = oc.check_step(data, hyper, clip, got, ctx)
        _say('RATIO %-34s %s' % (ctx, oc.fmt_ratios(r)))
        assert max(r.values()) <= 1.0
        if clip == 'off':
            off = got
        if clip == 'inactive' and off is not None:
            for k in ('p', 'g', 's1', 's2'):
                assert np.array_equal(oc.bits(got[k]), oc.bits(off[k])), '%s: %s differs from the run without clip' % (ctx, k)


@pytest.mark.parametrize('name', ['nulls', 'permuted'])
def test_dyadic_sgd_four_consecutive_steps(name):
    """SGD-momentum stays exact in fp32 over four steps of dyadic data: every step bit for bit"""
    case = next(c for c in oc.CASES if c.name == name)
    data = oc.make_data(case, oc.SGD, 'dyadic')
    hyper = oc.hyper_of(oc.SGD, 'dyadic')
    for step in range(4):
        ctx = '%s step %d' % (name, step + 1)
        got = run_step(data, hyper, 'off', ctx)
        oc.check_step(data, hyper, 'off', got, ctx)
        data = dict(data, p=got['p'], s1=got['s1'])


# ---- non-finite gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_norm', [1.0, 1e30], ids=['max_norm 1', 'max_norm 1e30'])
@pytest.mark.parametrize('bad', ['inf', 'nan'])
@pytest.mark.parametrize('kind,kname', oc.KINDS, ids=[k[1] for k in oc.KINDS])
def test_non_finite_gradient(kind, kname, bad, max_norm):
    """One Inf or one NaN gradient element under the clip, as torch.nn.utils.clip_grad_norm_ followed by the update treats it (held
    against torch in tests/test_optim_cases_cpu.py): an Inf norm gives the coefficient 0, so every gradient becomes 0 and the Inf
    one NaN; a NaN norm gives a NaN coefficient, so every gradient, state and parameter that has a gradient becomes NaN.
    clip_coef_kernel formed `c < 1 ? c : 1`, which turns a NaN norm into the coefficient 1: the step went through with the one NaN element
    and clean gradients elsewhere.  It now keeps the NaN."""
    case = next(c for c in oc.CASES if c.name == 'nulls')
    data = oc.make_data(case, kind, 'randn')
    g = data['g'].copy()
    g[300 + 4096] = np.inf if bad == 'inf' else np.nan                      # the one-element last chunk of tensor 1 has no gradient: the
    g[300 + 4097 + 17] = np.inf if bad == 'inf' else np.nan                 # value there must not count; this one (tensor 2) does
    data = dict(data, g=g)
    hyper = oc.hyper_of(kind, 'randn', None, data['t'], max_norm)
    ctx = 'nulls-%s-%s-%g' % (kname, bad, max_norm)
    got = run_twice(data, hyper, 'active', ctx)
    assert (np.isinf(got['norm']) if bad == 'inf' else np.isnan(got['norm'])), '%s: total norm %r' % (ctx, got['norm'])
    assert (got['coef'] == 0.0 if bad == 'inf' else np.isnan(got['coef'])), '%s: coefficient %r' % (ctx, got['coef'])
    r = oc.check_step(data, hyper, 'active', got, ctx)
    _say('RATIO %-34s %s' % (ctx, oc.fmt_ratios(r)))
    _, _, _, null = oc.elementwise(data['desc'])
    if bad == 'nan':
        assert np.isnan(got['p'][~null]).all() and np.isfinite(got['p'][null]).all()
    else:
        assert np.isnan(got['p'][~null]).sum() == 1 and np.isnan(got['p'][300 + 4097 + 17])


# ---- nnl_optim_patch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 7, 8, 9, 257])
def test_patch(n):
    """tensors[i].lr / .decay = dyn[2i] / dyn[2i + 1], hyper[0..8) = dyn[2n..): nothing else changes, bit for bit (n = 257 spans two blocks;
    below 8 tensors the hyper-parameters need threads of their own)"""
    from neuralnetworklibrary_amd._lib import check, lib, ptr, stream
    r = np.random.RandomState(n)
    item = oc.DESC.itemsize
    band = 64 * item
    image = r.randint(0, 256, band + n * item + 32 + band).astype(np.uint8)      # table and hyper, as FusedStep lays them out, in bands
    dyn = r.randn(2 * n + 8).astype(np.float32)
    dyn[0] = np.float32('nan')                                               # any bit pattern travels
    want = image.copy()
    table = want[band:band + n * item].view(oc.DESC)
    table['lr'], table['decay'] = dyn[0:2 * n:2], dyn[1:2 * n:2]
    want[band + n * item:band + n * item + 32] = dyn[2 * n:].view(np.uint8)
    for _ in range(2):
        dev = torch.from_numpy(image).to(DEV)
        d_dyn = torch.from_numpy(dyn).to(DEV)
        check(lib.nnl_optim_patch(ptr(dev[band:]), ptr(dev[band + n * item:]), ptr(d_dyn), n, stream()))
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, 'n = %d: byte %d (table starts at %d, hyper at %d) is %d, want %d; %d bytes differ' % (
            n, bad[0], band, band + n * item, got[bad[0]], want[bad[0]], bad.size)
        assert np.array_equal(d_dyn.cpu().numpy().view(np.int32), dyn.view(np.int32))
    before, after = image[band:band + n * item].view(oc.DESC), got[band:band + n * item].view(oc.DESC)
    for field in ('param', 'grad', 's1', 's2', 'numel'):
        assert np.array_equal(before[field], after[field])


# ---- FusedStep through Optimizer: five steps against the reference semantics in fp64 ---------------------------------------------------
class _Params(nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(t) for t in tensors])


def _bag(seed=0):
    """two layer groups, each with a regular and a 'bn' parameter group: no forward pass, the gradients are given.  reg1 holds a
    two-chunk vector, a channels_last 4-D tensor and a parameter that never gets a gradient."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    reg1 = _Params([rn(5000), rn(4, 6, 5, 5).contiguous(memory_format=torch.channels_last), rn(300)])
    reg2 = _Params([rn(37, 3), rn(1)])
    bn1, bn2 = _Params([rn(8) + 1]), _Params([rn(4097)])
    net = nn.Module()
    net.layer_groups = [nn.ModuleList([reg1, bn1]), nn.ModuleList([reg2, bn2])]
    net.groups = nn.ModuleList(net.layer_groups)
    net.param_groups = [reg1, reg2, bn1, bn2]
    return net


NO_GRAD = 2                                      # index, among net.parameters(), of the parameter without a gradient


def _grads(net, steps, seed=1):
    "per step, per parameter: contiguous fp32 gradients with |g| >= 0.05 (Adam's g / sqrt(v) does not amplify noise then)"
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        gs = []
        for i, p in enumerate(net.parameters()):
            r = torch.randn(p.shape, generator=g)
            gs.append(None if i == NO_GRAD else (torch.sign(r) * (0.05 + r.abs())).contiguous())
        out.append(gs)
    return out


def _optimizer(net, opt_name):
    from neuralnetworklibrary_amd.General.Learner import opt_dict
    from neuralnetworklibrary_amd.General.Optimizer import Optimizer
    return Optimizer(opt_dict[opt_name], net)


def _one_step(o, net, gs, dev, dtype, lr, kw):
    o.set_params(lr, **kw)
    for p, g in zip(net.parameters(), gs):
        p.grad = None if g is None else g.to(device=dev, dtype=dtype)
    o.step()


SCHEDULE = [[1e-2 * (i + 1), 3e-2 / (i + 1)] for i in range(5)]               # per step: one lr per layer group
CONFIGS = [
    ('SGD_Mom', dict(wd=[1e-2, 3e-2], bn_wd=True, clip=3.0, momentum=0.8)),
    ('SGD_Mom', dict(wd=1e-2, bn_wd=False, clip=None)),
    ('SGD', dict(wd=[1e-1, 2e-1], bn_wd=True, clip=None)),
    ('Adam', dict(wd=[1e-2, 5e-2], bn_wd=True, clip=5.0, betas=(0.8, 0.99))),
    ('Adam', dict(wd=1e-2, bn_wd=False, clip=1e9)),
]


def _reference_run(opt_name, kw, grads, schedule=SCHEDULE, seed=0):
    "the same steps in fp64 on the CPU: torch.optim after the decoupled decay and clip_grad_norm_ (Optimizer's torch path)"
    net = _bag(seed).double()
    o = _optimizer(net, opt_name)
    for gs, lr in zip(grads, schedule):
        _one_step(o, net, gs, 'cpu', torch.float64, lr, kw)
    assert o._fused is False
    return net, o


def _compare(net, ref, what):
    worst = 0.0
    for i, (p, q) in enumerate(zip(net.parameters(), ref.parameters())):
        assert_close(p, q, *oc.TOL_PROJECT, '%s: parameter %d' % (what, i))
        err = (p.detach().cpu().double() - q.detach()).abs()
        worst = max(worst, float((err / (oc.TOL_PROJECT[1] + oc.TOL_PROJECT[0] * q.detach().abs())).max()))
    _say('RATIO %-34s p %.3f of rtol 2e-5 / atol 1e-5' % (what, worst))


@pytest.mark.parametrize('opt_name,kw', CONFIGS, ids=['sgd-clip', 'sgd-nobnwd', 'sgd-mom0', 'adam-clip', 'adam-nobnwd-clip-inactive'])
def test_five_steps_through_optimizer(opt_name, kw):
    grads = _grads(_bag(), 5)
    ref, oref = _reference_run(opt_name, kw, grads)
    net = _bag().to(DEV)
    cl = list(net.parameters())[1]
    assert cl.is_contiguous(memory_format=torch.channels_last) and not cl.is_contiguous()
    o = _optimizer(net, opt_name)
    for gs, lr in zip(grads, SCHEDULE):
        _one_step(o, net, gs, DEV, torch.float32, lr, kw)
        assert cl.grad.stride() == cl.stride(), 'the gradient of a channels_last parameter was not re-laid like the parameter'
    assert o._fused is not None and o._fused is not False and o._fused.steps == 5, 'the fused HIP optimizer did not run'
    _compare(net, ref, '%s %s' % (opt_name, sorted(kw)))
    # the gradients that are left: clipped, in the parameter's layout, equal values
    for i, (p, q) in enumerate(zip(net.parameters(), ref.parameters())):
        if i == NO_GRAD:
            assert p.grad is None
        else:
            assert_close(p.grad, q.grad, 1e-5, 1e-7, 'gradient %d after the step' % i)
    if not kw['clip']:
        assert torch.equal(cl.grad.cpu(), grads[-1][1]), 'values of the re-laid gradient'


def test_loaded_adam_state_continues():
    """three steps of torch Adam in fp64, its state_dict loaded into the fused optimizer, two more steps there: as five steps in fp64.  The
    loaded per-parameter step counters all advance and the bias corrections are those of steps 4 and 5."""
    kw = dict(wd=[1e-2, 5e-2], bn_wd=True, clip=5.0, betas=(0.8, 0.99))
    grads = _grads(_bag(), 5)
    ref5, _ = _reference_run('Adam', kw, grads)
    ref3, o3 = _reference_run('Adam', kw, grads[:3])
    net = _bag().to(DEV)
    net.load_state_dict(ref3.state_dict())
    assert all(p.dtype == torch.float32 for p in net.parameters())
    o = _optimizer(net, 'Adam')
    o.opt.load_state_dict(copy.deepcopy(o3.opt.state_dict()))
    loaded = [o.opt.state[p] for i, p in enumerate(net.parameters()) if i != NO_GRAD]
    assert all(float(st['step']) == 3.0 and st['exp_avg'].dtype == torch.float32 and st['exp_avg'].is_cuda for st in loaded)
    assert len({id(st['step']) for st in loaded}) == len(loaded), 'a loaded state has a counter of its own per parameter'
    for gs, lr in zip(grads[3:], SCHEDULE[3:]):
        _one_step(o, net, gs, DEV, torch.float32, lr, kw)
    assert o._fused is not None and o._fused is not False and o._fused.steps == 2
    assert [float(st['step']) for st in loaded] == [5.0] * len(loaded)
    _compare(net, ref5, 'Adam, state loaded at step 3')


@pytest.mark.parametrize('opt_name,extra', [('Adam', dict(betas=[(0.9, 0.99), (0.8, 0.999)])), ('SGD_Mom', dict(momentum=[0.9, 0.5]))],
                         ids=['adam-betas', 'sgd-momentum'])
def test_hyper_parameters_per_group_take_the_torch_path(opt_name, extra):
    """betas / momentum differ between the layer groups: no single fused launch (uniform_hyper() is false), torch's kernels run, and the
    result is still that of the reference semantics"""
    kw = dict(wd=[1e-2, 5e-2], bn_wd=True, clip=5.0, **extra)
    grads = _grads(_bag(), 5)
    ref, _ = _reference_run(opt_name, kw, grads)
    net = _bag().to(DEV)
    o = _optimizer(net, opt_name)
    for gs, lr in zip(grads, SCHEDULE):
        _one_step(o, net, gs, DEV, torch.float32, lr, kw)
    assert o._fused is not None and o._fused is not False and not o._fused.uniform_hyper() and o._fused.steps == 0
    if opt_name == 'Adam':
        # FusedStep creates the Adam states with ONE counter tensor for all parameters; torch bumps every parameter's counter, which took
        # that tensor to 30 in five steps (and the bias corrections with it) until Optimizer.step() gave each state a counter of its own
        counters = [float(o.opt.state[p]['step']) for i, p in enumerate(net.parameters()) if i != NO_GRAD]
        assert counters == [5.0] * len(counters), 'step counters after five steps of torch Adam: %s' % counters
    _compare(net, ref, '%s per-group hyper-parameters' % opt_name)


# ---- run-ahead: the host enqueues four eager steps while the GPU has not begun the first -----------------------------------------------
def test_four_eager_steps_enqueued_ahead_of_the_gpu():
    """Optimizer.step() four times, with four different lr / wd, and no host synchronisation, behind filler work that keeps the stream busy
    until all four are enqueued.  Every step uploads its table (lr, decay, bias corrections, gradient pointers) from a pinned staging
    buffer with an asynchronous copy: a buffer the host rewrites before its copy has run hands a later step's values to an earlier one.
    With two alternating buffers and no event that is what happened here (parameter 0 off by 4.0e-2 after the four steps); FusedStep now
    takes the buffer from a ring of eight and waits for the event behind a slot's last copy before it rewrites the slot."""
    kw = lambda i: dict(wd=[1e-2 * (i + 1), 5e-2 / (i + 1)], bn_wd=True, clip=5.0, betas=(0.8, 0.99))
    grads = _grads(_bag(), 5)
    ref = _bag().double()
    oref = _optimizer(ref, 'Adam')
    for i, (gs, lr) in enumerate(zip(grads, SCHEDULE)):
        _one_step(oref, ref, gs, 'cpu', torch.float64, lr, kw(i))

    def warm():
        "a net after step 1, synchronised: the fused stepper and its pinned buffers exist"
        net = _bag().to(DEV)
        o = _optimizer(net, 'Adam')
        _one_step(o, net, grads[0], DEV, torch.float32, SCHEDULE[0], kw(0))
        dev_grads = [[None if g is None else g.to(DEV) for g in gs] for gs in grads]
        torch.cuda.synchronize()
        return net, o, dev_grads

    def four_steps(net, o, dev_grads):
        for i in range(1, 5):
            o.set_params(SCHEDULE[i], **kw(i))
            for p, g in zip(net.parameters(), dev_grads[i]):
                p.grad = None if g is None else g.clone()               # (the clip writes into it)
            o.step()

    # calibration, once: host time of enqueuing the four steps; GPU time of one filler matmul
    net, o, dg = warm()
    t0 = time.perf_counter()
    four_steps(net, o, dg)
    host_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    a = torch.randn(4096, 4096, device=DEV)
    b = torch.empty_like(a)
    torch.mm(a, a, out=b)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        torch.mm(a, a, out=b)
    e1.record()
    torch.cuda.synchronize()
    mm_s = e0.elapsed_time(e1) / 4 * 1e-3
    n_fill = int(np.ceil(20 * host_s / mm_s)) + 2
    assert n_fill <= 2000, 'enqueuing four steps took %.1f ms on the host: not a run the filler can cover' % (host_s * 1e3)

    net, o, dg = warm()
    done = torch.cuda.Event()
    for _ in range(n_fill):
        torch.mm(a, a, out=b)
    done.record()
    four_steps(net, o, dg)
    still_busy = not done.query()
    torch.cuda.synchronize()
    _say('run-ahead: four steps enqueued in %.2f ms on the host, filler %d matmuls of %.2f ms' % (host_s * 1e3, n_fill, mm_s * 1e3))
    assert still_busy, 'not the case meant'
    assert o._fused is not None and o._fused is not False and o._fused.steps == 5
    _compare(net, ref, 'four eager steps ahead of the GPU')
