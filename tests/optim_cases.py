"""The case table of the optimizer-step C-ABI sweep (tests/test_optim_abi_gpu.py, tests/test_optim_cases_cpu.py) and its fp64 reference.

A plain module: no fixtures, nothing from the library.  The reference restates, in numpy fp64, the header comment of nnl_optim_step
(include/nnl.h): decoupled weight decay, global-norm clip with write-back, SGD-momentum and Adam; tests/test_optim_cases_cpu.py holds
it against torch.optim + torch.nn.utils.clip_grad_norm_ in fp64.

csrc/optim.hip maps workgroup c to the piece (chunk_tensor[c], chunk_off[c]) of nnl_optim_chunk_elems() = 4096 elements; 256 threads
stride over a piece; clip_coef_kernel is ONE block of 256 threads striding over the n_chunks partial sums.  Every case below exists for
a regime of those loops and names it; facts() derives the regime from the table alone (plus the two run settings a case carries:
momentum and which clip settings it runs), REGIMES holds the predicates, and the CPU test checks every claim and that no regime is left
without a case.

Data modes:
  dyadic  p integer in [-8, 8], g in [-4, 4] (Adam: nonzero), lr / decay / momentum from {0.25, 0.5, 0.75}.  SGD-momentum is then exact
          in fp32 for four consecutive steps (every value a multiple of 4^-k below 2^7; the library is built with -ffp-contract=off), and
          Adam for the first step from zero state with beta1 = 0.5, beta2 = 0.75, bc1 = 0.5, sqrt(bc2) = 0.5, eps = 0: m = g/2, v = g^2/4,
          the update exactly +-0.5*lr/bc1.  Comparisons are bit for bit: a wrong offset, tail, tensor index, lr or decay shows as a
          difference, not as a rounding.  Sums of squares stay below 2^24 per piece, so the norm is float(sqrt(exact sum)) bit for bit too.
          With the clip ACTIVE the coefficient is no dyadic number and the randn bounds apply.
  randn   one step from random fp32 state, every 5th element with zero state and every 7th with |g| about 1e-6, every tensor with a
          learning rate and a decay of its own, bias corrections of step 1, 7 or 1000.  Elementwise bounds against the fp64 reference
          (U = 2^-24; each is the count of fp32 roundings in the kernel's expression plus slack):
            Adam  m:   4U(|b1 m0| + |w1 g|)            v: 6U v*
                  p:   4U(|p0 decay| + |U*|) + 16U (lr/bc1)(|b1 m0| + |w1 g|)/d*      d* = sqrt(v*)/sqrt_bc2 + eps, U* the exact update
            SGD   buf: 3U(|mom buf0| + |g|)
                  p:   4U(|p0 decay| + |lr buf*|) + 4U lr(|mom buf0| + |g|)

With the clip on, the checks are chained so that each bound stays that of ONE operation: the returned norm against sqrt of the fp64 sum
of squares (rtol norm_rtol(), below), the returned coefficient against min(1, max_norm / (returned norm + 1e-6)) to 4U relative, the
written-back gradient against g * returned coefficient to 4U|g|, and the update against the reference fed with the written-back
gradient (the value the kernel itself used).  NaN and Inf positions are compared, so the same chain covers non-finite gradients.

Measured on an MI355X, max err / bound over the whole sweep (tests/test_optim_abi_gpu.py prints them per case):
  randn, Adam   m 0.487   v 0.459   p 0.494   norm 0.016   coefficient 0.296   written-back gradient 0.083
  randn, SGD    buf 0.650           p 0.492   norm 0.013   coefficient 0.304   written-back gradient 0.125
  dyadic        every parameter, state, gradient and norm bit for bit; with the clip active coefficient 0.148, gradient 0.042
  one Inf / NaN gradient element: NaN and Inf in the reference's places, the finite rest p 0.463, m 0.234, v 0.151, buf 0.315
  through Optimizer (five steps, rtol 2e-5 / atol 1e-5): 0.013 of the tolerance at most
"""
import collections

import numpy as np

U = 2.0 ** -24                                   # unit roundoff of fp32 (round to nearest)
CHUNK = 4096                                     # nnl_optim_chunk_elems(), asserted by the CPU test
COEF_BLOCK = 256                                 # threads of clip_coef_kernel
STEP_BLOCK = 256                                 # threads of sqnorm_partial_kernel / optim_step_kernel
MAX_ELEMS = 2 * 1024 * 1024                      # no case is larger
DESC = np.dtype([('param', '<u8'), ('grad', '<u8'), ('s1', '<u8'), ('s2', '<u8'), ('numel', '<i8'), ('lr', '<f4'), ('decay', '<f4')])
SGD, ADAM = 0, 1
KINDS = [(SGD, 'sgd'), (ADAM, 'adam')]
CLIPS = ('off', 'active', 'inactive')
MODES = ('dyadic', 'randn')
QUARTERS = (0.25, 0.5, 0.75)
TOL_PROJECT = (2e-5, 1e-5)                       # (rtol, atol) of tests/test_optim_gpu.py::test_fused_matches_torch_path

# null: tensor index -> 'decay' (grad == NULL, decay != 1) or 'keep' (grad == NULL, decay == 1); order: None or 'shuffled'; momentum:
# None (the mode's own) or 0.0; clips: the clip settings the case runs
Case = collections.namedtuple('Case', 'name sizes null order momentum clips regimes')


def cdiv(a, b):
    return -(-a // b)


# ---- the tables -----------------------------------------------------------------------------------------------------------------
def build_table(sizes, chunk=CHUNK, order=None):
    """(desc, chunk_tensor, chunk_off): desc has fused_optim._DESC's dtype with numel filled in, param / grad / s1 / s2 = 1 (any
    non-NULL value; the caller writes the pointers, 0 into grad for a tensor without one) and lr = decay = 0; the chunk table lists every
    piece of every tensor once, tensor by tensor, or in the order given (a permutation of the pieces)."""
    desc = np.zeros(len(sizes), dtype=DESC)
    ct, co = [], []
    for t, n in enumerate(sizes):
        assert n > 0
        desc[t] = (1, 1, 1, 1, n, 0.0, 0.0)
        for off in range(0, n, chunk):
            ct.append(t)
            co.append(off)
    ct, co = np.asarray(ct, dtype=np.int32), np.asarray(co, dtype=np.int64)
    if order is not None:
        order = np.asarray(order)
        assert sorted(order.tolist()) == list(range(len(ct)))
        ct, co = ct[order], co[order]
    return desc, ct, co


Facts = collections.namedtuple('Facts', 'n_tensors numels chunks last_len n_chunks coef_passes coef_last_partial tiles null_decay '
                                        'null_keep distinct neighbours_differ permuted momentum clips')


def facts(desc, chunk_tensor, chunk_off, chunk=CHUNK, momentum=None, clips=()):
    """From the table alone: chunks[t] pieces of tensor t, the last of them last_len[t] long; n_chunks; coef_passes = how often thread 0
    of clip_coef_kernel loops, coef_last_partial = whether the last pass leaves threads without a partial sum; tiles = the pieces of
    every tensor cover [0, numel) exactly once; null_decay / null_keep = the tensors with grad == NULL and decay != 1 / == 1; distinct =
    no two tensors share an lr or a decay; neighbours_differ = tensor t and t + 1 differ in both; permuted = the chunk table is not in
    tensor-by-tensor order.  momentum and clips are the two run settings of the case, passed through."""
    n = len(desc)
    numels = [int(v) for v in desc['numel']]
    ct, co = np.asarray(chunk_tensor), np.asarray(chunk_off)
    chunks, last_len, tiles = [], [], True
    for t in range(n):
        offs = sorted(int(o) for o in co[ct == t])
        chunks.append(len(offs))
        tiles = tiles and offs == list(range(0, numels[t], chunk))
        last_len.append(numels[t] - offs[-1] if offs else 0)
    n_chunks = len(ct)
    lr, decay = desc['lr'].tolist(), desc['decay'].tolist()
    null = [t for t in range(n) if desc['grad'][t] == 0]
    live = [t for t in range(n) if t not in null or decay[t] != 1.0]
    canonical = build_table(numels, chunk)
    return Facts(n, numels, chunks, last_len, n_chunks, cdiv(n_chunks, COEF_BLOCK), n_chunks % COEF_BLOCK != 0, tiles,
                 [t for t in null if decay[t] != 1.0], [t for t in null if decay[t] == 1.0],
                 n > 1 and len(set(lr)) == n and len({decay[t] for t in live}) == len(live),
                 n > 1 and all(lr[t] != lr[t + 1] and decay[t] != decay[t + 1] for t in range(n - 1)),
                 not (np.array_equal(ct, canonical[1]) and np.array_equal(co, canonical[2])), momentum, tuple(clips))


def _has(f, numel):
    return numel in f.numels


REGIMES = collections.OrderedDict([
    ('numel = 1', lambda f: _has(f, 1)),
    ('numel < 256: idle lanes', lambda f: any(1 < n < STEP_BLOCK for n in f.numels)),
    ('numel = 4095', lambda f: _has(f, 4095) and f.last_len[f.numels.index(4095)] == 4095),
    ('numel = 4096', lambda f: _has(f, 4096) and f.chunks[f.numels.index(4096)] == 1),
    ('numel = 4097: last chunk of one element', lambda f: _has(f, 4097) and f.chunks[f.numels.index(4097)] == 2
     and f.last_len[f.numels.index(4097)] == 1),
    ('numel = 3*4096 + 17', lambda f: _has(f, 3 * 4096 + 17) and f.chunks[f.numels.index(3 * 4096 + 17)] == 4
     and f.last_len[f.numels.index(3 * 4096 + 17)] == 17),
    ('n_chunks = 1', lambda f: f.n_chunks == 1),
    ('n_chunks > 256, not a multiple: coef loop twice, last pass partial',
     lambda f: f.n_chunks > COEF_BLOCK and f.coef_passes == 2 and f.coef_last_partial and f.n_tensors >= 250),
    ('n_chunks = 256: one full coef pass', lambda f: f.n_chunks == COEF_BLOCK and not f.coef_last_partial),
    ('grad NULL mid-table, decay != 1', lambda f: any(0 < t < f.n_tensors - 1 for t in f.null_decay)),
    ('grad NULL, decay == 1', lambda f: bool(f.null_keep)),
    ('grad NULL tensor of several chunks', lambda f: any(f.chunks[t] > 1 for t in f.null_decay + f.null_keep)),
    ('every tensor its own lr and decay', lambda f: f.distinct and f.n_tensors >= 3),
    ('chunk table permuted', lambda f: f.permuted and f.tiles and f.n_chunks >= 6),
    ('momentum == 0', lambda f: f.momentum == 0.0),
    ('clip off', lambda f: 'off' in f.clips),
    ('clip active', lambda f: 'active' in f.clips),
    ('clip inactive', lambda f: 'inactive' in f.clips),
])


def _mixed_sizes(n):
    "n small tensors of mixed sizes, some of two chunks"
    return [(37 * i * i + 11 * i) % 5000 + 1 for i in range(n)]


CASES = [
    Case('one', [1], {}, None, None, CLIPS, ['numel = 1', 'n_chunks = 1']),
    Case('idle', [200, 7, 255], {}, None, None, CLIPS, ['numel < 256: idle lanes', 'every tensor its own lr and decay']),
    Case('edges', [4095, 4096, 4097], {}, None, None, CLIPS,
         ['numel = 4095', 'numel = 4096', 'numel = 4097: last chunk of one element', 'clip off', 'clip active', 'clip inactive']),
    Case('tail17', [3 * 4096 + 17, 5], {}, None, None, CLIPS, ['numel = 3*4096 + 17']),
    Case('many', _mixed_sizes(300), {}, None, None, CLIPS,
         ['n_chunks > 256, not a multiple: coef loop twice, last pass partial', 'every tensor its own lr and decay', 'numel = 1']),
    Case('full256', [255 * 4096, 4096], {}, None, None, CLIPS, ['n_chunks = 256: one full coef pass', 'numel = 4096']),
    Case('nulls', [300, 4097, 50, 4096, 9], {1: 'decay', 3: 'keep'}, None, None, CLIPS,
         ['grad NULL mid-table, decay != 1', 'grad NULL, decay == 1', 'grad NULL tensor of several chunks']),
    Case('permuted', [4097, 1, 2 * 4096 + 3, 255, 4096], {2: 'decay'}, 'shuffled', None, CLIPS,
         ['chunk table permuted', 'grad NULL tensor of several chunks', 'numel = 1']),
    Case('mom0', [4097, 33, 1], {}, None, 0.0, CLIPS, ['momentum == 0', 'numel = 4097: last chunk of one element']),
]


def case_id(c):
    return c.name


def rates(case, mode):
    """fp32 (lr, decay) per tensor.  dyadic: quarters, neighbours differ in both (period 9: all nine pairs).  randn: all distinct."""
    n = len(case.sizes)
    i = np.arange(n)
    if mode == 'dyadic':
        lr = np.asarray(QUARTERS, dtype=np.float32)[i % 3]
        decay = np.asarray(QUARTERS, dtype=np.float32)[(i + i // 3) % 3]
    else:
        lr = (1e-3 * 1.015 ** i).astype(np.float32)
        decay = (1.0 - 3e-4 * (i + 1)).astype(np.float32)
    for t, how in case.null.items():
        if how == 'keep':
            decay[t] = 1.0
    return lr, decay


def table_of(case, mode):
    """the case's table: numel, lr, decay, grad = 0 for its gradient-less tensors"""
    desc, ct, co = build_table(case.sizes)
    if case.order == 'shuffled':
        desc, ct, co = build_table(case.sizes, order=np.random.RandomState(5).permutation(len(ct)))
    desc['lr'], desc['decay'] = rates(case, mode)
    for t in case.null:
        desc['grad'][t] = 0
    return desc, ct, co


def facts_of(case, mode='randn'):
    return facts(*table_of(case, mode), momentum=case.momentum, clips=case.clips)


def elementwise(desc):
    "per element of the concatenated tensors: tensor index, lr, decay (fp64, widened from the table's fp32), has-no-gradient"
    tid = np.repeat(np.arange(len(desc)), desc['numel'])
    return tid, desc['lr'].astype(np.float64)[tid], desc['decay'].astype(np.float64)[tid], (desc['grad'] == 0)[tid]


# ---- hyper-parameters and data ---------------------------------------------------------------------------------------------------
ADAM_STEPS = (1, 7, 1000)


def hyper_of(kind, mode, momentum=None, t=1, max_norm=0.0):
    """the 8 fp32 values nnl_optim_step reads: {momentum | 1 - beta1, beta1, beta2, eps, bc1, sqrt(bc2), max_norm, 1 - beta2}; 1 - beta and the
    bias corrections are formed in double and rounded once, as FusedStep does"""
    if kind == SGD:
        mom = (0.75 if mode == 'dyadic' else 0.9) if momentum is None else momentum
        h = [mom, 0., 0., 0., 1., 1., max_norm, 0.]
    elif mode == 'dyadic':
        h = [0.5, 0.5, 0.75, 0.0, 0.5, 0.5, max_norm, 0.25]
    else:
        b1, b2 = 0.9, 0.999
        h = [1.0 - b1, b1, b2, 1e-8, 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t), max_norm, 1.0 - b2]
    return np.asarray(h, dtype=np.float32)


def make_data(case, kind, mode, seed=0):
    """fp32 state of the concatenated tensors: p, g, s1, s2 (a gradient-less tensor has values in g all the same: nothing may read or
    write them), the table, and the Adam step t of the bias corrections"""
    idx = [c.name for c in CASES].index(case.name) if case in CASES else 99
    r = np.random.RandomState(1000 * seed + 10 * idx + kind)
    n = int(sum(case.sizes))
    assert n <= MAX_ELEMS
    i = np.arange(n)
    if mode == 'dyadic':
        p = r.randint(-8, 9, n)
        if kind == ADAM:
            g = r.randint(1, 5, n) * (2 * r.randint(0, 2, n) - 1)
            s1, s2 = np.zeros(n), np.zeros(n)
        else:
            g = r.randint(-4, 5, n)
            g[0] = 3                                                       # (a norm of zero cannot be clipped)
            s1, s2 = r.randint(-4, 5, n), np.zeros(n)
    else:
        p, g = r.randn(n), r.randn(n)
        g[(i + 3) % 7 == 0] *= 1e-6
        zero = (i + 2) % 5 == 0
        if kind == ADAM:
            s1, s2 = 0.1 * r.randn(n), (0.1 * r.randn(n)) ** 2
        else:
            s1, s2 = 0.5 * r.randn(n), np.zeros(n)
        s1[zero] = 0
        s2[zero] = 0
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    desc, ct, co = table_of(case, mode)
    return dict(p=f(p), g=f(g), s1=f(s1), s2=f(s2), desc=desc, chunk_tensor=ct, chunk_off=co, t=ADAM_STEPS[idx % 3], mode=mode, kind=kind)


def grad_norm(data):
    "sqrt of the fp64 sum of squares over the tensors that have a gradient"
    _, _, _, null = elementwise(data['desc'])
    g = data['g'].astype(np.float64)[~null]
    with np.errstate(all='ignore'):
        return float(np.sqrt(np.sum(g * g)))


def max_norm_of(data, clip):
    "fp32 max_norm that makes the clip active (half the norm) or inactive (twice the norm plus one); 0 with the clip off"
    if clip == 'off':
        return np.float32(0.0)
    nrm = grad_norm(data)
    return np.float32(0.5 * nrm if clip == 'active' else 2.0 * nrm + 1.0)


def norm_rtol(desc, chunk=CHUNK):
    """rtol of the returned total norm: 4U * (1 + depth), depth = ceil(log2(longest piece with a gradient)).  The kernel squares in fp32
    (one rounding), then adds in fp32, all on non-negative numbers: ceil(L/256) squares per thread, 6 butterfly levels within a wave,
    2 more additions across the 4 waves.  The partial sums are added in fp64; the square root halves the relative error of the sum and the
    cast to fp32 adds one U.  norm_roundings() counts the roundings on the longest path (an addition of zero is exact); the CPU test holds
    it below this rtol for every piece length."""
    live = [min(int(n), chunk) for n, g in zip(desc['numel'], desc['grad']) if g != 0]
    depth = int(np.ceil(np.log2(max(live)))) if live else 0
    return 4 * U * (1 + depth)


def norm_roundings(L):
    "worst-case relative error of the returned norm, in units of U, for a longest piece of L elements (see norm_rtol)"
    clog2 = lambda n: int(np.ceil(np.log2(n)))
    serial = cdiv(L, STEP_BLOCK) - 1
    wave = min(6, clog2(min(L, 64)))
    across = clog2(cdiv(min(L, STEP_BLOCK), 64))
    return (1 + serial + wave + across) / 2.0 + 1


# ---- the fp64 reference of one step (include/nnl.h, "K8: fused multi-tensor Optimizer.step") ----------------------------------------
def clip_ref(g, null, max_norm):
    """(total norm, coefficient) of the gradients that exist: coef = min(1, max_norm / (norm + 1e-6)), NaN where the norm is NaN
    (torch.nn.utils.clip_grad_norm_ clamps, and a clamp keeps NaN)"""
    with np.errstate(all='ignore'):
        gg = g[~null]
        norm = np.sqrt(np.sum(gg * gg))
        return norm, coef_from_norm(norm, max_norm)


def coef_from_norm(norm, max_norm):
    with np.errstate(all='ignore'):
        return np.minimum(1.0, np.float64(max_norm) / (np.float64(norm) + 1e-6))         # np.minimum propagates NaN


def step_ref(kind, p0, g, s1_0, s2_0, lr, decay, null, hyper, use_clip, g_applied=None):
    """One nnl_optim_step in fp64 over the concatenated tensors.  p0, g, s1_0, s2_0, lr, decay: fp64 per element (lr / decay / hyper:
    the fp32 values the kernel is given, widened); null: per element, the tensor has no gradient.  g_applied: the clipped gradient to
    use instead of g * coef (the GPU test passes what the kernel wrote back, after checking it).

      no gradient:  p = p0 * decay, nothing else changes
      clip:         g <- g * coef, written back
      SGD:          buf = momentum * buf0 + g (momentum == 0: buf is not touched, d = g);  p = p0 * decay - lr * buf
      Adam:         m = beta1 m0 + w1 g;  v = beta2 v0 + w2 g^2;  p = p0 * decay - (lr / bc1) * m / (sqrt(v) / sqrt_bc2 + eps)

    Returns p, g, s1, s2, norm, coef (None without clip) and the bounds of the module docstring as p_bound, s1_bound, s2_bound."""
    h = np.asarray(hyper, dtype=np.float64)
    norm = coef = None
    with np.errstate(all='ignore'):
        gc = g
        if use_clip:
            norm, coef = clip_ref(g, null, h[6])
            gc = np.where(null, g, g * coef if g_applied is None else g_applied)
        pd = p0 * decay
        if kind == SGD:
            mom = h[0]
            a, b = mom * s1_0, gc
            buf = a + b
            upd = lr * buf
            s1 = s1_0.copy() if mom == 0.0 else np.where(null, s1_0, buf)
            s2 = s2_0.copy()
            s1_bound = 3 * U * (np.abs(a) + np.abs(b))
            s2_bound = np.zeros_like(p0)
            p_bound = 4 * U * (np.abs(pd) + np.abs(upd)) + 4 * U * lr * (np.abs(a) + np.abs(b))
        else:
            w1, b1, b2, eps, bc1, sbc2, w2 = h[0], h[1], h[2], h[3], h[4], h[5], h[7]
            a, b = b1 * s1_0, w1 * gc
            m = a + b
            v = b2 * s2_0 + w2 * gc * gc
            d = np.sqrt(v) / sbc2 + eps
            upd = (lr / bc1) * (m / d)
            s1, s2 = np.where(null, s1_0, m), np.where(null, s2_0, v)
            s1_bound = 4 * U * (np.abs(a) + np.abs(b))
            s2_bound = 6 * U * v
            p_bound = 4 * U * (np.abs(pd) + np.abs(upd)) + 16 * U * (lr / bc1) * (np.abs(a) + np.abs(b)) / d
        p = np.where(null, pd, pd - upd)
        p_bound = np.where(null, 4 * U * np.abs(pd), p_bound)
        s1_bound, s2_bound = np.where(null, 0.0, s1_bound), np.where(null, 0.0, s2_bound)
        if kind == SGD and h[0] == 0.0:
            s1_bound = np.zeros_like(p0)
    return dict(p=p, g=gc, s1=s1, s2=s2, norm=norm, coef=coef, p_bound=p_bound, s1_bound=s1_bound, s2_bound=s2_bound)


def reference(data, hyper, use_clip, g_applied=None):
    "step_ref on a make_data() state"
    _, lr, decay, null = elementwise(data['desc'])
    d = lambda k: data[k].astype(np.float64)
    return step_ref(data['kind'], d('p'), d('g'), d('s1'), d('s2'), lr, decay, null, hyper, use_clip,
                    None if g_applied is None else np.asarray(g_applied, dtype=np.float64))


# ---- comparing a result with the reference -----------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _ratio(got, want, bound, what, ctx):
    """max |got - want| / bound over the elements where both are numbers; NaN must sit in the same places, an infinity must be equal.
    A bound of zero asks for equality."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        i = int(np.argmax(gn != wn))
        raise AssertionError('%s: %s has NaN in other places than the reference, first at %d: got %r, want %r' % (ctx, what, i, got[i], want[i]))
    with np.errstate(all='ignore'):
        err = np.where(got == want, 0.0, np.abs(got - want))
        err = np.where(gn, 0.0, err)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
        bound = np.where(np.isfinite(want), bound, 0.0)                     # (an infinite bound would let anything through)
        bad = ~(err <= bound) & ~gn
        if bad.any():
            i = int(np.argmax(np.where(bad, np.where(np.isfinite(err), err, np.inf), -1.0)))
            raise AssertionError('%s: %s off at element %d of %d: got %r, want %r, |diff| %.3e, bound %.3e (%d elements out of bound)' %
                                 (ctx, what, i, err.size, got[i], want[i], err[i], bound[i], int(bad.sum())))
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    return float(r.max()) if r.size else 0.0


def _same_bits(got, want, what, ctx):
    if not np.array_equal(bits(got), bits(want)):
        i = int(np.argmax(bits(got) != bits(want)))
        raise AssertionError('%s: %s differs bitwise, first at element %d: got %r, want %r (%d elements differ)' %
                             (ctx, what, i, np.ravel(got)[i], np.ravel(want)[i], int((bits(got) != bits(want)).sum())))


def check_step(data, hyper, clip, got, ctx=''):
    """A result `got` = dict(p, g, s1, s2 fp32 over the concatenated tensors; norm, coef fp32 scalars with the clip on) of ONE step from
    `data` against the fp64 reference.  Exact (bit for bit) in dyadic mode unless the clip is active, else within the derived bounds.
    Returns the ratios max err / bound (an exact comparison reports 0)."""
    use_clip = clip != 'off'
    exact = data['mode'] == 'dyadic' and clip != 'active'
    _, _, _, null = elementwise(data['desc'])
    g0 = data['g'].astype(np.float64)
    ratios = collections.OrderedDict()
    g_applied = None
    if use_clip:
        norm64, _ = clip_ref(g0, null, hyper[6])
        norm, coef = np.float32(got['norm']), np.float32(got['coef'])
        if data['mode'] == 'dyadic' and np.isfinite(norm64):
            _same_bits(norm, np.float32(norm64), 'total norm', ctx)
            ratios['norm'] = 0.0
        else:
            ratios['norm'] = _ratio([norm], [norm64], norm_rtol(data['desc']) * abs(norm64), 'total norm', ctx)
        want_coef = coef_from_norm(np.float64(norm), np.float64(hyper[6]))
        if clip == 'inactive':
            assert want_coef == 1.0 and bits(coef) == bits(np.float32(1.0)), '%s: inactive clip, coefficient %r is not exactly 1' % (ctx, coef)
            ratios['coef'] = 0.0
        else:
            ratios['coef'] = _ratio([coef], [want_coef], 4 * U * abs(want_coef), 'clip coefficient', ctx)
        if clip == 'active':
            assert not want_coef >= 1.0, '%s: not the case meant: the clip is not active (coefficient %r)' % (ctx, want_coef)
        with np.errstate(all='ignore'):
            want_g = np.where(null, g0, g0 * np.float64(coef))
        if bits(coef) == bits(np.float32(1.0)):
            _same_bits(got['g'], data['g'], 'gradient after a clip by 1', ctx)
            ratios['g'] = 0.0
        else:
            ratios['g'] = _ratio(got['g'], want_g, np.where(null, 0.0, 4 * U * np.abs(g0)), 'written-back gradient', ctx)
        g_applied = got['g']
    else:
        _same_bits(got['g'], data['g'], 'gradient (no clip: must come back unchanged)', ctx)
    ref = reference(data, hyper, use_clip, g_applied)
    # what must not change at all
    if null.any():
        _same_bits(got['s1'][null], data['s1'][null], 'state1 of a gradient-less tensor', ctx)
        _same_bits(got['s2'][null], data['s2'][null], 'state2 of a gradient-less tensor', ctx)
        _same_bits(got['g'][null], data['g'][null], 'memory next to a NULL gradient', ctx)
        keep = null & (elementwise(data['desc'])[2] == 1.0)
        _same_bits(got['p'][keep], data['p'][keep], 'parameter of a gradient-less tensor with decay 1', ctx)
    if data['kind'] == SGD:
        _same_bits(got['s2'], data['s2'], 'state2 under SGD', ctx)
        if hyper[0] == 0.0:
            _same_bits(got['s1'], data['s1'], 'momentum buffer with momentum == 0', ctx)
    for k in ('p', 's1', 's2'):
        if exact:
            want32 = ref[k].astype(np.float32)
            assert np.array_equal(want32.astype(np.float64), ref[k]), '%s: dyadic %s is not exact in fp32' % (ctx, k)
            _same_bits(got[k], want32, k, ctx)
            ratios[k] = 0.0
        else:
            ratios[k] = _ratio(got[k], ref[k], ref[k + '_bound'], k, ctx)
    return ratios


def fmt_ratios(r):
    return '  '.join('%s %.3f' % kv for kv in r.items())


if __name__ == '__main__':
    for c in CASES:
        f = facts_of(c)
        print(case_id(c), f.n_tensors, 'tensors', f.n_chunks, 'chunks;', '; '.join(c.regimes))
