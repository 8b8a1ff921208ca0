"""The case table of the LSTM C-ABI sweep (tests/test_lstm_abi_gpu.py, tests/test_lstm_cases_cpu.py) and its fp64 reference.

A plain module: no fixtures, nothing from the library.  reference() restates, in torch fp64 and as an explicit time loop, the header
comment of K5 (include/nnl.h): gates_t = gx_t + h_{t-1} W_hh^T, gate order i, f, g, o, c_t = s(f) c_{t-1} + s(i) tanh(g),
h_t = s(o) tanh(c_t), and its BPTT with optional dy, dhT, dcT; tests/test_lstm_cases_cpu.py holds it against torch.nn.LSTM under
autograd.

nnl_lstm_fwd / nnl_lstm_bwd pick one of six routes (csrc/lstm.hip): the persistent forward (lstm_persist.hip, templated on U units per
workgroup), the per-timestep forward (sf k slices), the 2-D partitioned BPTT (lstm_bptt2.hip, templated on NT column tiles and PB polls
per batch), the first persistent BPTT (U again), and the per-timestep backward in two launches or fused (sb slabs, summed by add_slabs
in 16-, 8-, 4-wide loops and a tail).  Which one runs follows from NNL_LSTM_PERSIST, NNL_LSTM_FUSED_BWD, err_flag and the host plan
that nnl_debug_lstm_plan reports.  Every case below exists for regimes of those kernels and names them; REGIMES holds the predicates over
(case, plan), and the CPU test checks every claim, that no regime is left without a case and that every instantiation the planner
can reach is named by a case.

Observed on an MI355X (tests/test_lstm_abi_gpu.py, worst over the cases of a route; the forward as max |err| / (atol + rtol |ref|),
the gradients as max |err| / (atol_rel max|ref| + rtol |ref|): 1.0 would be the tolerance):
  route                y      cy     gates  | route                dgates dh0    dc0
  lstm_persist_fwd     0.006  0.010  0.013  | lstm_bptt2           0.001  0.002  0.001
  lstm_step_fwd        0.009  0.016  0.027  | lstm_persist_bwd     0.002  0.005  0.002
                                            | lstm_step_bwd        0.001  0.004  0.001
                                            | lstm_step_bwd:fused  0.000  0.001  0.001
                                            | library fwd -> bwd   0.001  0.003  0.001
The largest absolute errors: gates 3.1e-07 (lstm_step_fwd, 2x65x1027), dh0 2.2e-06 (lstm_persist_bwd, 2x64x1027).  No case needed
the fp32 rule of check(): at T <= 9 an fp32 recurrence is two orders of magnitude inside the project's tolerances, so these bounds
catch a wrong or missing term (tests/test_lstm_cases_cpu.py shows five such), not a lost bit.
"""
import collections
import functools

import torch

# the project's tolerances (tests/test_text.py::test_lstm_full_size_recurrence_vs_torch_and_bitwise_repeatable)
TOL_FWD = (1e-4, 1e-5)                           # y, cy, gates: rtol, atol
TOL_GRAD = (1e-3, 1e-4)                          # dgates, dh0, dc0: rtol, atol = 1e-4 * max|reference|
FP32_FACTOR = 3.0                                # an output beyond its tolerance passes if err <= 3 * (error of the same recurrence in
                                                 # torch fp32 on the CPU) + the tolerance's atol: an fp32 kernel cannot be asked to beat fp32
SENTINEL = 12345.0                               # outputs are pre-filled with it; no LSTM output of these inputs comes near it

FWD_OUT = ('y', 'cy', 'gates')
BWD_OUT = ('dgates', 'dh0', 'dc0')

Case = collections.namedtuple('Case', 'T B H fwd bwd persist fused nulls regimes')
Plan = collections.namedtuple('Plan', 'Hp Gp tf tb sf sb persist_ok U NWG bptt2_ok NT PB KG NG')


def cdiv(a, b):
    return -(-a // b)


def C(T, B, H, fwd, bwd, persist, regimes, fused=0, nulls=()):
    """fwd: 'persist' | 'step';  bwd: 'bptt2' | 'persist' | 'step' | 'fused';  persist: NNL_LSTM_PERSIST;  nulls: of 'dy', 'dhT', 'dcT',
    'err_flag'"""
    return Case(T, B, H, fwd, bwd, persist, fused, tuple(nulls), regimes)


# ---- which route a call takes (lstm.hip: nnl_lstm_fwd, nnl_lstm_bwd) ------------------------------------------------------------------
def routes(case, p):
    """(fwd, bwd) route kinds the entry points take for this case under plan p"""
    flag = 'err_flag' not in case.nulls
    fwd = 'persist' if (case.persist & 1) and flag and p.persist_ok else 'step'
    if (case.persist & 4) and flag and p.bptt2_ok:
        bwd = 'bptt2'
    elif (case.persist & 2) and flag and p.persist_ok:
        bwd = 'persist'
    else:
        bwd = 'fused' if case.fused == 1 else 'step'
    return fwd, bwd


def route_notes(case, p):
    """the route notes (nnl_debug_route_collect) the two calls must leave"""
    fwd, bwd = routes(case, p)
    nf = 'lstm_persist_fwd<%d>@%d' % (p.U, p.NWG) if fwd == 'persist' else 'lstm_step_fwd@%d' % p.sf
    nb = {'bptt2': 'lstm_bptt2<%d,%d>@%dx%d' % (p.NT, p.PB, p.KG, p.NG), 'persist': 'lstm_persist_bwd<%d>@%d' % (p.U, p.NWG),
          'step': 'lstm_step_bwd@%d' % p.sb, 'fused': 'lstm_step_bwd:fused@%d' % p.sb}[bwd]
    return nf, nb


def instantiations(case, p):
    """the template instantiations the two calls run"""
    fwd, bwd = routes(case, p)
    out = set()
    if fwd == 'persist':
        out.add('lstm_persist_fwd_kernel<%d>' % p.U)
    if bwd == 'persist':
        out.add('lstm_persist_bwd_kernel<%d>' % p.U)
    if bwd == 'bptt2':
        out.add('lstm_bptt2_kernel<%d,%d>' % (p.NT, p.PB))
    return out


def reachable_instantiations(p):
    """what some choice of switches runs at a shape with plan p"""
    out = set()
    if p.persist_ok:
        out |= {'lstm_persist_fwd_kernel<%d>' % p.U, 'lstm_persist_bwd_kernel<%d>' % p.U}
    if p.bptt2_ok:
        out.add('lstm_bptt2_kernel<%d,%d>' % (p.NT, p.PB))
    return out


# what the library instantiates (lstm_persist.hip kMaxU = 5; lstm_bptt2.hip NT 1..6 x PB 8 / 16 without <6,16>), and what else its
# planners' ranges would allow (U up to 8 by the 4U <= 32 gate columns, <6,16>): asserted unreachable for B <= 128, H <= 4096
INSTANTIATED = {'lstm_persist_%s_kernel<%d>' % (d, u) for d in ('fwd', 'bwd') for u in range(1, 6)} | \
               {'lstm_bptt2_kernel<%d,%d>' % (nt, pb) for nt in range(1, 7) for pb in (8, 16)} - {'lstm_bptt2_kernel<6,16>'}
UNREACHABLE = {'lstm_persist_%s_kernel<%d>' % (d, u) for d in ('fwd', 'bwd') for u in (6, 7, 8)} | {'lstm_bptt2_kernel<6,16>'}


# ---- regimes: named predicates over (case, plan) ---------------------------------------------------------------------------------------
def _fwd(c, p):
    return routes(c, p)[0]


def _bwd(c, p):
    return routes(c, p)[1]


def _fwd_kg(p):
    return p.Hp // 32                            # k groups (4 k each) per wave of the persistent forward: chunks of 12, then a rest


def _slab_loops(n):
    """how add_slabs walks n slabs: (16-wide passes, 8-wide, 4-wide, tail)"""
    a, n = divmod(n, 16)
    b, n = divmod(n, 8)
    c, n = divmod(n, 4)
    return a, b, c, n


REGIMES = collections.OrderedDict()
for _u in range(1, 6):
    REGIMES['persistent fwd U = %d' % _u] = lambda c, p, u=_u: _fwd(c, p) == 'persist' and p.U == u
    REGIMES['persistent bwd U = %d' % _u] = lambda c, p, u=_u: _bwd(c, p) == 'persist' and p.U == u
for _u in (3, 4, 5):
    REGIMES['last workgroup ragged, U = %d, fwd and bwd' % _u] = lambda c, p, u=_u: (
        _fwd(c, p) == 'persist' and _bwd(c, p) == 'persist' and p.U == u and 0 < c.H - (p.NWG - 1) * u < u)
REGIMES.update([
    ('persistent fwd k loop: rest only', lambda c, p: _fwd(c, p) == 'persist' and _fwd_kg(p) < 12),
    ('persistent fwd k loop: single request batch (13 groups)', lambda c, p: _fwd(c, p) == 'persist' and _fwd_kg(p) == 13),
    ('persistent fwd k loop: one chunk plus rest', lambda c, p: _fwd(c, p) == 'persist' and 13 < _fwd_kg(p) < 24),
    ('persistent fwd k loop: rotated chunks plus rest', lambda c, p: _fwd(c, p) == 'persist' and _fwd_kg(p) >= 24 and _fwd_kg(p) % 12),
    ('persistent kernels, all 64 batch lanes', lambda c, p: _fwd(c, p) == 'persist' and _bwd(c, p) == 'persist' and c.B == 64),
])
for _nt, _pb in [(1, 8), (1, 16), (2, 8), (2, 16), (3, 8), (3, 16), (4, 8), (4, 16), (5, 8), (5, 16), (6, 8)]:
    REGIMES['lstm_bptt2<%d,%d>' % (_nt, _pb)] = lambda c, p, nt=_nt, pb=_pb: _bwd(c, p) == 'bptt2' and (p.NT, p.PB) == (nt, pb)
REGIMES.update([
    ('bptt2 exchange ring wrapped twice', lambda c, p: _bwd(c, p) == 'bptt2' and c.T >= 9),
    ('bptt2 all four streams live (B = 64)', lambda c, p: _bwd(c, p) == 'bptt2' and c.B == 64),
    ('bptt2 streams without batch rows (B <= 16)', lambda c, p: _bwd(c, p) == 'bptt2' and c.B <= 16),
    ('bptt2 one live row in a stream', lambda c, p: _bwd(c, p) == 'bptt2' and c.B % 16 == 1 and c.B > 1),
    ('bptt2 behind a per-timestep forward', lambda c, p: _bwd(c, p) == 'bptt2' and _fwd(c, p) == 'step'),
    ('per-timestep, B <= 64', lambda c, p: _fwd(c, p) == 'step' and _bwd(c, p) == 'step' and c.B <= 64),
    ('per-timestep, B = 65', lambda c, p: _fwd(c, p) == 'step' and _bwd(c, p) == 'step' and c.B == 65),
    ('per-timestep, B = 128', lambda c, p: _fwd(c, p) == 'step' and _bwd(c, p) == 'step' and c.B == 128),
    ('fused bwd, B = 65', lambda c, p: _bwd(c, p) == 'fused' and c.B == 65),
    ('sf = 1', lambda c, p: _fwd(c, p) == 'step' and p.sf == 1),
    ('sf = 1 by the tile count', lambda c, p: _fwd(c, p) == 'step' and p.sf == 1 and p.tf > 128 and p.Hp > 32),
    ('sf > 1', lambda c, p: _fwd(c, p) == 'step' and p.sf > 1),
    ('sb = 32: the 16-wide loop alone', lambda c, p: _bwd(c, p) == 'step' and p.sb == 32),
    ('sb: 16 + 4 + tail', lambda c, p: _bwd(c, p) == 'step' and _slab_loops(p.sb)[0] == 1 and _slab_loops(p.sb)[1] == 0 and
     _slab_loops(p.sb)[2] == 1 and _slab_loops(p.sb)[3] > 0),
    ('sb: 16 + 8 + 4 + tail', lambda c, p: _bwd(c, p) == 'step' and min(_slab_loops(p.sb)) > 0),
    ('sb: 8 + 4 + tail', lambda c, p: _bwd(c, p) == 'step' and _slab_loops(p.sb)[0] == 0 and min(_slab_loops(p.sb)[1:]) > 0),
    ('sb < 4', lambda c, p: _bwd(c, p) == 'step' and p.sb < 4),
    ('4H % 32 != 0 on the per-timestep path', lambda c, p: _fwd(c, p) == 'step' and _bwd(c, p) in ('step', 'fused') and (4 * c.H) % 32 != 0),
    ('H < 16', lambda c, p: c.H < 16),
    ('fused bwd', lambda c, p: _bwd(c, p) == 'fused' and c.T > 1),
    ('two-launch bwd', lambda c, p: _bwd(c, p) == 'step' and c.T > 1),
    ('err_flag NULL, switches ask for persistent', lambda c, p: 'err_flag' in c.nulls and c.persist == 5 and p.persist_ok and p.bptt2_ok and
     routes(c, p) == ('step', 'step')),
    ('dy, dhT and dcT all NULL', lambda c, p: {'dy', 'dhT', 'dcT'} <= set(c.nulls)),
    ('dhT and dcT NULL', lambda c, p: set(c.nulls) - {'err_flag'} == {'dhT', 'dcT'}),
])
for _r in ('persist', 'step'):
    REGIMES['T = 1: %s fwd' % _r] = lambda c, p, r=_r: c.T == 1 and _fwd(c, p) == r
for _r in ('bptt2', 'persist', 'step', 'fused'):
    REGIMES['T = 1: %s bwd' % _r] = lambda c, p, r=_r: c.T == 1 and _bwd(c, p) == r
    for _n in ('dy', 'dhT', 'dcT'):
        REGIMES['%s NULL alone: %s bwd' % (_n, _r)] = lambda c, p, r=_r, n=_n: set(c.nulls) - {'err_flag'} == {n} and _bwd(c, p) == r

CASES = [
    # the persistent kernels, forward and first BPTT (NNL_LSTM_PERSIST = 3)
    C(2, 3, 5, 'persist', 'persist', 3, ['persistent fwd U = 1', 'persistent bwd U = 1', 'H < 16', 'persistent fwd k loop: rest only']),
    C(2, 5, 257, 'persist', 'persist', 3, ['persistent fwd U = 2', 'persistent bwd U = 2']),
    C(5, 9, 401, 'persist', 'persist', 3, ['persistent fwd k loop: single request batch (13 groups)', 'dy NULL alone: persist bwd'],
      nulls=['dy']),
    C(5, 7, 515, 'persist', 'persist', 3, ['persistent fwd U = 3', 'persistent bwd U = 3', 'last workgroup ragged, U = 3, fwd and bwd',
                                          'persistent fwd k loop: one chunk plus rest']),
    C(2, 20, 771, 'persist', 'persist', 3, ['persistent fwd U = 4', 'persistent bwd U = 4', 'last workgroup ragged, U = 4, fwd and bwd',
                                           'persistent fwd k loop: rotated chunks plus rest']),
    C(2, 64, 1027, 'persist', 'persist', 3, ['persistent fwd U = 5', 'persistent bwd U = 5', 'last workgroup ragged, U = 5, fwd and bwd',
                                            'persistent kernels, all 64 batch lanes']),
    C(1, 4, 37, 'persist', 'persist', 3, ['T = 1: persist fwd', 'T = 1: persist bwd']),
    C(2, 4, 37, 'persist', 'persist', 3, ['dhT NULL alone: persist bwd'], nulls=['dhT']),
    C(2, 6, 13, 'persist', 'persist', 3, ['dcT NULL alone: persist bwd'], nulls=['dcT']),
    # the 2-D partitioned BPTT (NNL_LSTM_PERSIST = 5): every (NT, PB) plan2 returns, at the smallest H that has it
    C(2, 3, 1, 'persist', 'bptt2', 5, ['lstm_bptt2<1,16>', 'bptt2 streams without batch rows (B <= 16)']),
    C(9, 3, 25, 'persist', 'bptt2', 5, ['lstm_bptt2<1,8>', 'bptt2 exchange ring wrapped twice']),
    C(1, 3, 25, 'persist', 'bptt2', 5, ['T = 1: bptt2 bwd']),
    C(5, 17, 185, 'persist', 'bptt2', 5, ['lstm_bptt2<2,8>', 'bptt2 one live row in a stream']),
    C(9, 64, 233, 'persist', 'bptt2', 5, ['lstm_bptt2<2,16>', 'bptt2 exchange ring wrapped twice', 'bptt2 all four streams live (B = 64)']),
    C(2, 33, 569, 'persist', 'bptt2', 5, ['lstm_bptt2<3,8>', 'bptt2 one live row in a stream']),
    C(2, 20, 593, 'persist', 'bptt2', 5, ['lstm_bptt2<3,16>']),
    C(2, 5, 825, 'persist', 'bptt2', 5, ['lstm_bptt2<4,8>']),
    C(2, 16, 929, 'persist', 'bptt2', 5, ['lstm_bptt2<4,16>']),
    C(2, 12, 1081, 'persist', 'bptt2', 5, ['lstm_bptt2<5,8>']),
    C(9, 20, 1169, 'persist', 'bptt2', 5, ['lstm_bptt2<5,16>', 'bptt2 exchange ring wrapped twice']),
    C(2, 8, 1337, 'step', 'bptt2', 5, ['lstm_bptt2<6,8>', 'bptt2 behind a per-timestep forward']),
    C(2, 6, 17, 'persist', 'bptt2', 5, ['dy NULL alone: bptt2 bwd'], nulls=['dy']),
    C(5, 20, 100, 'persist', 'bptt2', 5, ['dhT NULL alone: bptt2 bwd'], nulls=['dhT']),
    C(2, 4, 37, 'persist', 'bptt2', 5, ['dcT NULL alone: bptt2 bwd'], nulls=['dcT']),
    # the per-timestep path (NNL_LSTM_PERSIST = 0, or a batch over 64 whatever the switch says)
    C(5, 20, 250, 'step', 'step', 0, ['per-timestep, B <= 64', 'sf > 1', 'sb = 32: the 16-wide loop alone', 'two-launch bwd',
                                      '4H % 32 != 0 on the per-timestep path']),
    C(5, 20, 161, 'step', 'step', 0, ['sb: 16 + 4 + tail']),
    C(2, 20, 225, 'step', 'step', 0, ['sb: 16 + 8 + 4 + tail']),
    C(2, 20, 100, 'step', 'step', 0, ['sb: 8 + 4 + tail', 'dy NULL alone: step bwd'], nulls=['dy']),
    C(2, 3, 5, 'step', 'step', 0, ['sf = 1', 'sb < 4', 'H < 16', 'dhT NULL alone: step bwd'], nulls=['dhT']),
    C(5, 6, 17, 'step', 'step', 0, ['sb < 4', 'dcT NULL alone: step bwd'], nulls=['dcT']),
    C(2, 65, 1027, 'step', 'step', 5, ['per-timestep, B = 65', 'sf = 1 by the tile count']),
    C(5, 65, 37, 'step', 'step', 5, ['per-timestep, B = 65', 'dhT and dcT NULL'], nulls=['dhT', 'dcT']),
    C(2, 128, 100, 'step', 'step', 5, ['per-timestep, B = 128']),
    C(1, 4, 37, 'step', 'step', 0, ['T = 1: step fwd', 'T = 1: step bwd']),
    C(1, 4, 37, 'step', 'fused', 0, ['T = 1: fused bwd'], fused=1),
    C(5, 20, 161, 'step', 'fused', 0, ['fused bwd', '4H % 32 != 0 on the per-timestep path'], fused=1),
    C(2, 65, 100, 'step', 'fused', 5, ['fused bwd, B = 65', 'dy NULL alone: fused bwd'], fused=1, nulls=['dy']),
    C(2, 6, 17, 'step', 'fused', 0, ['dhT NULL alone: fused bwd'], fused=1, nulls=['dhT']),
    C(5, 3, 5, 'step', 'fused', 0, ['dcT NULL alone: fused bwd'], fused=1, nulls=['dcT']),
    C(2, 8, 64, 'step', 'step', 5, ['err_flag NULL, switches ask for persistent'], nulls=['err_flag']),
    C(2, 5, 13, 'step', 'step', 0, ['dy, dhT and dcT all NULL'], nulls=['dy', 'dhT', 'dcT']),
]
# library forward chained into library backward: one case per backward route
CHAINED = [CASES[3], CASES[13], CASES[25]]


def case_id(c):
    return '%dx%dx%d-%s-%s-p%d%s%s' % (c.T, c.B, c.H, c.fwd, c.bwd, c.persist, '-fused' if c.fused else '',
                                       ''.join('-no_' + n for n in c.nulls))


# ---- data ------------------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """fp32 CPU tensors, scaled as tests/test_text.py scales them (gates stay out of saturation): gx [T,B,4H], w_hh [4H,H], h0, c0
    [B,H], dy [T,B,H], dhT, dcT [B,H] (None where the case passes NULL)"""
    T, B, H = case.T, case.B, case.H
    g = torch.Generator().manual_seed(100003 * T + 1009 * B + H + 7 * len(case.nulls))
    d = dict(gx=torch.randn(T, B, 4 * H, generator=g) * 0.5, w_hh=torch.randn(4 * H, H, generator=g) / H ** 0.5,
             h0=torch.randn(B, H, generator=g) * 0.1, c0=torch.randn(B, H, generator=g) * 0.1,
             dy=torch.randn(T, B, H, generator=g), dhT=torch.randn(B, H, generator=g), dcT=torch.randn(B, H, generator=g))
    for n in ('dy', 'dhT', 'dcT'):
        if n in case.nulls:
            d[n] = None
    return d


# ---- the reference (include/nnl.h, "K5: recurrence of one weight-dropped LSTM layer") ------------------------------------------------
def lstm_forward(gx, w_hh, h0, c0):
    """y, cy [T,B,H] and the ACTIVATED gates [T,B,4H] (i, f, g, o), in the dtype of the arguments"""
    T, H = gx.shape[0], w_hh.shape[1]
    h, c = h0, c0
    ys, cs, gs = [], [], []
    for t in range(T):
        pre = gx[t] + h @ w_hh.t()
        i, f, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
        g = torch.tanh(pre[:, 2 * H:3 * H])
        c = f * c + i * g
        h = o * torch.tanh(c)
        ys.append(h); cs.append(c); gs.append(torch.cat([i, f, g, o], 1))
    return torch.stack(ys), torch.stack(cs), torch.stack(gs)


def lstm_backward(dy, dhT, dcT, gates, cy, c0, w_hh):
    """dgates [T,B,4H] (gradient of the PRE-activation gates = d gx), dh0, dc0 [B,H]; dy, dhT, dcT may be None (= 0)"""
    T, B, H = cy.shape
    dh = torch.zeros_like(c0) if dhT is None else dhT
    dc = torch.zeros_like(c0) if dcT is None else dcT
    dgs = [None] * T
    for t in range(T - 1, -1, -1):
        if dy is not None:
            dh = dh + dy[t]
        i, f, g, o = (gates[t][:, k * H:(k + 1) * H] for k in range(4))
        c_prev = c0 if t == 0 else cy[t - 1]
        tc = torch.tanh(cy[t])
        dcn = dc + dh * o * (1 - tc * tc)
        dgs[t] = torch.cat([dcn * g * (i * (1 - i)), dcn * c_prev * (f * (1 - f)), dcn * i * (1 - g * g), dh * tc * (o * (1 - o))], 1)
        dc = dcn * f
        dh = dgs[t] @ w_hh
    return torch.stack(dgs), dh, dc


def recurrence(case, dtype):
    d = make_inputs(case)
    x = {k: (None if v is None else v.to(dtype)) for k, v in d.items()}
    y, cy, gates = lstm_forward(x['gx'], x['w_hh'], x['h0'], x['c0'])
    dgates, dh0, dc0 = lstm_backward(x['dy'], x['dhT'], x['dcT'], gates, cy, x['c0'], x['w_hh'])
    return dict(y=y, cy=cy, gates=gates, dgates=dgates, dh0=dh0, dc0=dc0)


@functools.lru_cache(maxsize=None)
def reference(case_index):
    """the fp64 reference of CASES[case_index] (inputs rounded to fp32 first); computed once, shared, never modified"""
    return recurrence(CASES[case_index], torch.float64)


# ---- the shared checker --------------------------------------------------------------------------------------------------------------------
def tolerance(name, ref):
    """(rtol, atol) of output `name` against its fp64 reference"""
    if name in FWD_OUT:
        return TOL_FWD
    return TOL_GRAD[0], TOL_GRAD[1] * float(ref.abs().max())


def check(out, ref, case, cpu32=None):
    """out: CPU tensors (or numpy arrays) by name — any of y, cy, gates, dh0, dc0 [fp32] and dgates_pad [T,B,Gp] — as an entry point
    left them in buffers pre-filled with SENTINEL (dgates_pad: zero in its columns >= 4H).  Asserts, per output: no element kept the
    fill value, the pad columns of dgates_pad are still exactly zero, and every element is within the project's tolerance of ref.
    cpu32: a callable that returns the same recurrence computed in fp32 on the CPU; an output beyond its tolerance is then accepted if
    max err <= FP32_FACTOR * (max err of cpu32) + atol.  Returns {name: (worst err / tolerance, max err, max err of cpu32 or None)}."""
    G = 4 * case.H
    report = {}
    for name, got in out.items():
        got = torch.as_tensor(got)
        ctx = '%s: %s' % (case_id(case), name)
        if name == 'dgates_pad':
            pad = got[..., G:]
            assert int((pad != 0).sum()) == 0, '%s: %d pad elements (columns >= 4H) are not exactly zero' % (ctx, int((pad != 0).sum()))
            got, name = got[..., :G], 'dgates'
        want = ref[name]
        assert tuple(got.shape) == tuple(want.shape), '%s: shape %s, want %s' % (ctx, tuple(got.shape), tuple(want.shape))
        kept = int((got == SENTINEL).sum())
        assert kept == 0, '%s: %d elements were never written (still the sentinel)' % (ctx, kept)
        assert bool(torch.isfinite(got).all()), '%s: not finite' % ctx
        rtol, atol = tolerance(name, want)
        err = (got.double() - want).abs()
        lim = atol + rtol * want.abs()
        ratio, e32 = float((err / lim.clamp_min(1e-300)).max()), None      # (an all-zero reference, atol = 0: exactly zero is asked)
        if ratio > 1.0 and cpu32 is not None:
            e32 = float((cpu32()[name].double() - want).abs().max())
            ok = float(err.max()) <= FP32_FACTOR * e32 + atol
        else:
            ok = ratio <= 1.0
        if not ok:
            i = tuple(int(v) for v in torch.unravel_index((err / lim.clamp_min(1e-300)).argmax(), err.shape))
            raise AssertionError('%s: max abs err %.3e (%.2f x the tolerance), worst at %s: got %r, want %r, tolerance there %.3e%s' % (
                ctx, float(err.max()), ratio, i, float(got[i]), float(want[i]), float(lim[i]),
                '' if e32 is None else '; fp32 on the CPU errs by %.3e' % e32))
        report[name] = (ratio, float(err.max()), e32)
    return report


if __name__ == '__main__':
    for c in CASES:
        print(case_id(c), '; '.join(c.regimes))
