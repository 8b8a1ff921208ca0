"""tests/optim_cases.py without a GPU: every case reaches the launch regime it names, no regime is left without a case, the fp64 one-step
reference agrees with torch.optim.SGD / Adam after the reference's decoupled decay and clip_grad_norm_ (non-finite gradients included),
a float32 numpy model of the documented formula passes every comparison of tests/test_optim_abi_gpu.py, seven wrong variants of it fail
them, and nnl_optim_step / nnl_optim_patch refuse bad arguments before any HIP call."""
import numpy as np
import pytest
import torch

import optim_cases as oc

F32 = np.float32


# ---- the case table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', oc.CASES, ids=oc.case_id)
def test_case_reaches_its_regimes(case):
    f = oc.facts_of(case, 'randn')
    assert f.tiles and f.n_chunks == sum(oc.cdiv(n, oc.CHUNK) for n in case.sizes) and sum(case.sizes) <= oc.MAX_ELEMS
    assert f.chunks == [oc.cdiv(n, oc.CHUNK) for n in case.sizes]
    assert f.last_len == [n - (oc.cdiv(n, oc.CHUNK) - 1) * oc.CHUNK for n in case.sizes]
    assert f.coef_passes == oc.cdiv(f.n_chunks, 256) and f.coef_last_partial == (f.n_chunks % 256 != 0)
    assert case.regimes, 'a case names the regime it exists for'
    for name in case.regimes:
        assert oc.REGIMES[name](f), '%s does not reach "%s": %s' % (case.name, name, f)
    # the dyadic table has the same structure, and neighbouring tensors differ in lr and in decay wherever both update
    fd = oc.facts_of(case, 'dyadic')
    assert (fd.chunks, fd.last_len, fd.n_chunks, fd.permuted, fd.null_keep, fd.null_decay) == \
           (f.chunks, f.last_len, f.n_chunks, f.permuted, f.null_keep, f.null_decay)
    assert f.n_tensors == 1 or f.null_keep or fd.neighbours_differ
    assert f.n_tensors == 1 or f.distinct
    for lr, decay in (oc.rates(case, 'dyadic'),):
        assert set(lr.tolist()) <= set(oc.QUARTERS) and set(decay.tolist()) <= set(oc.QUARTERS) | {1.0}


def test_census_every_regime_has_a_case():
    claimed = {name for c in oc.CASES for name in c.regimes}
    assert claimed == set(oc.REGIMES), 'regimes without a case: %s' % sorted(set(oc.REGIMES) - claimed)
    assert len({c.name for c in oc.CASES}) == len(oc.CASES)
    assert all(set(c.clips) == set(oc.CLIPS) for c in oc.CASES)


def test_chunk_size_and_descriptor_layout():
    from neuralnetworklibrary_amd import fused_optim
    from neuralnetworklibrary_amd._lib import lib
    assert int(lib.nnl_optim_chunk_elems()) == oc.CHUNK
    assert oc.DESC == fused_optim._DESC and oc.DESC.itemsize == 48


def test_table_builder():
    desc, ct, co = oc.build_table([1, 4096, 4097, 9000])
    assert ct.dtype == np.int32 and co.dtype == np.int64 and desc.dtype == oc.DESC
    assert ct.tolist() == [0, 1, 2, 2, 3, 3, 3] and co.tolist() == [0, 0, 0, 4096, 0, 4096, 8192]
    f = oc.facts(desc, ct, co)
    assert f.chunks == [1, 1, 2, 3] and f.last_len == [1, 4096, 1, 808] and f.n_chunks == 7 and f.tiles and not f.permuted
    assert (f.coef_passes, f.coef_last_partial) == (1, True)
    d2, ct2, co2 = oc.build_table([1, 4096, 4097, 9000], order=[6, 0, 3, 2, 5, 1, 4])
    f2 = oc.facts(d2, ct2, co2)
    assert f2.permuted and f2.tiles and f2.chunks == f.chunks and f2.last_len == f.last_len
    assert not oc.facts(desc, ct[:-1], co[:-1]).tiles                        # a piece missing
    for n, want in ((256, (1, False)), (257, (2, True)), (512, (2, False))):
        f = oc.facts(*oc.build_table([n * oc.CHUNK]))
        assert (f.coef_passes, f.coef_last_partial) == want


def test_norm_rtol_covers_the_roundings_of_the_reduction():
    for L in list(range(1, 300)) + [511, 512, 513, 4095, 4096]:
        desc = oc.build_table([L])[0]
        assert oc.norm_roundings(L) * oc.U <= oc.norm_rtol(desc), L
    desc = oc.build_table([5000, 7])[0]
    assert oc.norm_rtol(desc) == 4 * oc.U * 13                               # pieces are 4096 long at most
    desc['grad'][0] = 0
    assert oc.norm_rtol(desc) == 4 * oc.U * 4                                # only 7 elements carry a gradient


@pytest.mark.parametrize('mode', oc.MODES)
@pytest.mark.parametrize('kind,kname', oc.KINDS, ids=[k[1] for k in oc.KINDS])
@pytest.mark.parametrize('case', oc.CASES, ids=oc.case_id)
def test_clip_settings_are_what_they_say(case, kind, kname, mode):
    data = oc.make_data(case, kind, mode)
    nrm = oc.grad_norm(data)
    assert nrm > 0
    assert oc.coef_from_norm(nrm, oc.max_norm_of(data, 'active')) < 0.75
    assert oc.coef_from_norm(nrm, oc.max_norm_of(data, 'inactive')) == 1.0
    if mode == 'randn':
        i = np.arange(data['g'].size)
        assert data['g'].size < 7 or (np.abs(data['g'][(i + 3) % 7 == 0]) < 1e-5).all()
        assert data['g'].size < 5 or ((data['s1'] == 0) & (data['s2'] == 0)).sum() >= data['g'].size // 5
        assert (data['g'] != 0).all()


# ---- the reference against torch in fp64 -------------------------------------------------------------------------------------------
def _torch_steps(kind, sizes, null, p0, g_steps, lrs, decays, momentum, betas, eps, max_norm):
    """torch.optim in fp64: per step the reference's decoupled decay, clip_grad_norm_, opt.step()"""
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    groups = [{'params': [p], 'lr': 0.0} for p in ps]
    opt = torch.optim.SGD(groups, momentum=momentum) if kind == oc.SGD else torch.optim.Adam(groups, betas=betas, eps=eps)
    out = []
    for gs, lr, decay in zip(g_steps, lrs, decays):
        for i, p in enumerate(ps):
            opt.param_groups[i]['lr'] = float(lr[i])
            p.grad = None if i in null else torch.from_numpy(gs[i].copy())
        with torch.no_grad():
            for p, d in zip(ps, decay):
                p.mul_(float(d))
        nrm = None
        if max_norm:
            nrm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        opt.step()
        out.append(([p.detach().numpy().copy() for p in ps], [None if p.grad is None else p.grad.numpy().copy() for p in ps], nrm))
    return out, opt, ps


# (non-finite gradients matter through the clip coefficient: they run with the clip on)
@pytest.mark.parametrize('max_norm,bad', [(None, None), (0.7, None), (1e6, None), (0.7, 'inf'), (0.7, 'nan'), (1e6, 'inf'), (1e6, 'nan')],
                         ids=['noclip', 'active', 'inactive', 'active-inf', 'active-nan', 'inactive-inf', 'inactive-nan'])
@pytest.mark.parametrize('kind,momentum', [(oc.SGD, 0.9), (oc.SGD, 0.0), (oc.ADAM, None)], ids=['sgd', 'sgd-mom0', 'adam'])
def test_reference_agrees_with_torch(kind, momentum, max_norm, bad):
    sizes, null = [5, 1, 300, 17], {1}
    r = np.random.RandomState(3)
    p0 = [r.randn(n) for n in sizes]
    steps = 3
    g_steps = [[r.randn(n) for n in sizes] for _ in range(steps)]
    if bad:
        g_steps[1][2][7] = np.inf if bad == 'inf' else np.nan
    lrs = [np.array([0.1, 0.2, 0.05, 0.3]) * (s + 1) for s in range(steps)]
    decays = [1 - 0.01 * lr for lr in lrs]
    b1, b2, eps = 0.9, 0.999, 1e-8
    want, _, _ = _torch_steps(kind, sizes, null, p0, g_steps, lrs, decays, momentum or 0.0, (b1, b2), eps, max_norm)

    tid = np.repeat(np.arange(len(sizes)), sizes)
    nul = np.isin(tid, list(null))
    p, s1, s2 = np.concatenate(p0), np.zeros(sum(sizes)), np.zeros(sum(sizes))
    for s in range(steps):
        t = s + 1
        h = [momentum, 0, 0, 0, 1, 1, max_norm or 0, 0] if kind == oc.SGD else \
            [1 - b1, b1, b2, eps, 1 - b1 ** t, np.sqrt(1 - b2 ** t), max_norm or 0, 1 - b2]
        ref = oc.step_ref(kind, p, np.concatenate(g_steps[s]), s1, s2, lrs[s][tid], decays[s][tid], nul, h, bool(max_norm))
        p, s1, s2 = ref['p'], ref['s1'], ref['s2']
        wp, wg, wn = want[s]
        np.testing.assert_allclose(p, np.concatenate(wp), rtol=1e-11, atol=1e-13, equal_nan=True)
        if max_norm:
            np.testing.assert_allclose(ref['norm'], wn, rtol=1e-13, equal_nan=True)
            live = ~nul
            np.testing.assert_allclose(ref['g'][live], np.concatenate([g for g in wg if g is not None]), rtol=1e-13, atol=0, equal_nan=True)
    if bad == 'nan':
        assert np.isnan(p[~nul]).all() and np.isfinite(p[nul]).all(), 'a NaN norm makes every gradient, hence every updated parameter, NaN'
    if bad == 'inf':
        assert np.isnan(p[~nul]).sum() == 1, 'an Inf norm zeroes the gradients; only Inf * 0 is NaN'


# ---- a float32 model of the documented formula, and wrong variants of it ------------------------------------------------------------------
MUTANTS = ['last element of a chunk skipped', "a chunk takes the next tensor's lr", 'no decay on a gradient-less tensor',
           'the norm misses a chunk', 'bias correction of step t - 1', '1 - beta2 formed in fp32', 'clipped gradients not written back']


def model32(data, hyper, clip, mutant=None):
    """nnl_optim_step as include/nnl.h documents it, in float32 numpy, chunk by chunk from the table (so that a mutant can get one chunk
    wrong).  Every operation is one correctly rounded fp32 operation, in the order of the header's formula."""
    desc, ct, co = data['desc'], data['chunk_tensor'], data['chunk_off']
    kind = data['kind']
    start = np.concatenate([[0], np.cumsum(desc['numel'])])
    p, g, s1, s2 = (data[k].copy() for k in ('p', 'g', 's1', 's2'))
    h = np.asarray(hyper, dtype=F32).copy()
    if mutant == 'bias correction of step t - 1':
        h[4:6] = oc.hyper_of(kind, data['mode'], t=data['t'] - 1)[4:6]
    w2 = F32(1) - h[2] if mutant == '1 - beta2 formed in fp32' else h[7]
    live = [c for c in range(len(ct)) if desc['grad'][ct[c]] != 0]
    # the chunk a mutant gets wrong: one that matters (not the smallest), whose tensor has a successor
    target = max((c for c in live if ct[c] + 1 < len(desc) or len(desc) == 1), key=lambda c: min(oc.CHUNK, desc['numel'][ct[c]] - co[c]))
    span = lambda c: (start[ct[c]] + co[c], start[ct[c]] + min(co[c] + oc.CHUNK, desc['numel'][ct[c]]))
    out = dict(norm=None, coef=None)
    coef = F32(1)
    with np.errstate(all='ignore'):
        if clip != 'off':
            partial = []
            for c in live:
                if mutant == 'the norm misses a chunk' and c == target:
                    continue
                a, b = span(c)
                partial.append(np.sum(g[a:b] * g[a:b], dtype=F32))
            total = F32(np.sqrt(np.sum(np.asarray(partial, dtype=np.float64))))
            coef = np.minimum(F32(1), h[6] / (total + F32(1e-6)))
            out.update(norm=total, coef=coef)
        for c in range(len(ct)):
            t = ct[c]
            a, b = span(c)
            lr, decay = F32(desc['lr'][t]), F32(desc['decay'][t])
            if c == target and mutant == 'last element of a chunk skipped':
                b -= 1
            if c == target and mutant == "a chunk takes the next tensor's lr":
                lr = F32(desc['lr'][(t + 1) % len(desc)])
            if desc['grad'][t] == 0:
                if mutant != 'no decay on a gradient-less tensor':
                    p[a:b] = p[a:b] * decay
                continue
            gc = g[a:b] * coef
            if clip != 'off' and mutant != 'clipped gradients not written back':
                g[a:b] = gc
            x = p[a:b] * decay
            if kind == oc.SGD:
                d = gc
                if h[0] != 0:
                    d = h[0] * s1[a:b] + gc
                    s1[a:b] = d
                x = x - lr * d
            else:
                m = h[1] * s1[a:b] + h[0] * gc
                v = h[2] * s2[a:b] + w2 * gc * gc
                s1[a:b], s2[a:b] = m, v
                x = x - (lr / h[4]) * (m / (np.sqrt(v) / h[5] + h[3]))
            p[a:b] = x
    assert all(v.dtype == F32 for v in (p, g, s1, s2))
    out.update(p=p, g=g, s1=s1, s2=s2)
    return out


def _setup(case, kind, mode, clip):
    data = oc.make_data(case, kind, mode)
    hyper = oc.hyper_of(kind, mode, case.momentum, data['t'], oc.max_norm_of(data, clip))
    return data, hyper


@pytest.mark.parametrize('clip', oc.CLIPS)
@pytest.mark.parametrize('mode', oc.MODES)
@pytest.mark.parametrize('kind,kname', oc.KINDS, ids=[k[1] for k in oc.KINDS])
@pytest.mark.parametrize('case', oc.CASES, ids=oc.case_id)
def test_reference_and_model_pass_every_comparison(case, kind, kname, mode, clip):
    data, hyper = _setup(case, kind, mode, clip)
    ctx = '%s-%s-%s-%s' % (case.name, kname, mode, clip)
    # the reference itself, rounded to fp32
    ref = oc.reference(data, hyper, clip != 'off')
    got = {k: ref[k].astype(F32) for k in ('p', 'g', 's1', 's2')}
    got.update(norm=None if ref['norm'] is None else F32(ref['norm']), coef=None if ref['coef'] is None else F32(ref['coef']))
    r = oc.check_step(data, hyper, clip, got, ctx + ' (reference in fp32)')
    assert max(r.values()) <= 0.6, r                  # one rounding of the result against bounds that count three and more
    # the fp32 model
    m = model32(data, hyper, clip)
    r = oc.check_step(data, hyper, clip, m, ctx + ' (fp32 model)')
    assert max(r.values()) <= 1.0
    if clip == 'inactive':                             # bit-identical to the run without clip
        off = model32(data, oc.hyper_of(kind, mode, case.momentum, data['t'], 0.0), 'off')
        for k in ('p', 'g', 's1', 's2'):
            assert np.array_equal(oc.bits(m[k]), oc.bits(off[k]))


def test_dyadic_sgd_is_exact_for_four_steps():
    case = next(c for c in oc.CASES if c.name == 'nulls')
    data = oc.make_data(case, oc.SGD, 'dyadic')
    hyper = oc.hyper_of(oc.SGD, 'dyadic')
    for step in range(4):
        m = model32(data, hyper, 'off')
        oc.check_step(data, hyper, 'off', m, 'step %d' % step)
        ref = oc.reference(data, hyper, False)
        for k in ('p', 's1'):
            assert np.array_equal(ref[k].astype(F32).astype(np.float64), ref[k]), 'step %d: %s is not exact in fp32' % (step, k)
        data = dict(data, p=m['p'], s1=m['s1'])


def _mutant_runs():
    """every mutant on four tables, both kinds; the decay mutant where there is a gradient-less tensor, the two Adam hyper-parameter
    mutants under Adam in randn mode (the dyadic hyper-parameters are exact either way)"""
    runs = []
    for name, mode in [('nulls', 'dyadic'), ('nulls', 'randn'), ('many', 'randn'), ('edges', 'dyadic')]:
        case = next(c for c in oc.CASES if c.name == name)
        for kind, kname in oc.KINDS:
            for mutant in MUTANTS:
                if mutant == 'no decay on a gradient-less tensor' and not case.null:
                    continue
                if mutant in ('bias correction of step t - 1', '1 - beta2 formed in fp32') and (kind == oc.SGD or mode == 'dyadic'):
                    continue
                runs.append((name, mode, kind, kname, mutant))
    return runs


@pytest.mark.parametrize('name,mode,kind,kname,mutant', _mutant_runs(), ids=['%s-%s-%s-%s' % (r[0], r[1], r[3], r[4]) for r in _mutant_runs()])
def test_mutants_of_the_model_fail(name, mode, kind, kname, mutant):
    case = next(c for c in oc.CASES if c.name == name)
    clip = 'active' if mutant in ('the norm misses a chunk', 'clipped gradients not written back') else 'off'
    data, hyper = _setup(case, kind, mode, clip)
    oc.check_step(data, hyper, clip, model32(data, hyper, clip), 'honest model')
    with pytest.raises(AssertionError):
        oc.check_step(data, hyper, clip, model32(data, hyper, clip, mutant), mutant)


# ---- argument checks: before any HIP call, so without a device ----------------------------------------------------------------------
def test_argument_checks():
    import ctypes
    from neuralnetworklibrary_amd._lib import lib
    buf = (ctypes.c_char * 256)()
    x = ctypes.cast(buf, ctypes.c_void_p)                                  # any non-NULL pointer: nothing is launched
    step = lambda *a: lib.nnl_optim_step(*a)
    good = [x, x, x, 1, 0, x, 0, None, None]

    def refused(args, word, fn=step):
        st = fn(*args)
        err = lib.nnl_last_error()
        assert st == -1 and word in err, (args, st, err)

    for i in (0, 1, 2, 5):                                                 # tensors, chunk_tensor, chunk_off, hyper
        a = list(good)
        a[i] = None
        refused(a, b'optim_step: bad table')
    for n in (0, -1, 1 << 31):
        refused(good[:3] + [n] + good[4:], b'optim_step: bad table')
    for kind in (2, -1):
        refused(good[:4] + [kind] + good[5:], b'kind must be 0 (SGD) or 1 (Adam)')
    refused(good[:6] + [1, None, None], b'clipping needs a workspace')
    patch = lambda *a: lib.nnl_optim_patch(*a)
    for a in ([None, x, x, 1, None], [x, None, x, 1, None], [x, x, None, 1, None], [x, x, x, 0, None], [x, x, x, -3, None],
              [x, x, x, 1 << 24, None]):
        refused(a, b'optim_patch: bad arguments', patch)
