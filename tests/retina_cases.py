"""The case table of the detection-loss C-ABI sweep (tests/test_retina_abi_gpu.py, tests/test_retina_cases_cpu.py), its inputs, its
reference and its tolerances.

A plain module: no fixtures, nothing from the library, nothing from the GPU.  It restates the header comment of K6 (include/nnl.h,
csrc/retina_loss.hip) twice:

  state      numpy fp32, operation by operation as the kernel does it: area = (x2-x1)*(y2-y1), iw = max(min(x2) - max(x1), 0),
             iou = inter / ((area_o + area_a) - inter), first maximum wins, > fp32(0.5) positive, < fp32(0.4) negative, else ignored
             (-2), no objects: all negative (-1).  The kernel's state and npos are compared with it EXACTLY.
  values     torch fp64 under autograd, given that state: inputs cast up from fp32, the constants 0.1, 0.2, 1e-4 and 1 - 1e-4 as their
             fp32 values cast up (so the inclusive ends of the clamp agree with the kernel), focal term written with p (not 1-(1-p)),
             Huber with its knee at 1/9, the means as the header states them.

restate32() is the same arithmetic in numpy fp32 (encode, focal gradient, Huber, forward terms).  It is no reference: the CPU test runs
it through check_forward / check_backward to prove that a correct fp32 evaluation fits the tolerances below before any kernel is judged
by them.

Launch regimes of csrc/retina_loss.hip the table is built around (REGIMES holds the predicates; coverage() lists the cases of each):
  class path   K % 4 != 0: one element per lane and step, the anchor of element e from int((e + .5) * (1/K)); K % 4 == 0: 16-byte pieces,
               the first kPre * 256 = 2048 of a chunk from registers fetched before the matching, the rest in a tail loop (K > 32)
  chunks       256 anchors per block; a last chunk of fewer; more than 64 chunks make the finalize's lanes loop
  batch        the finalize's wave w owns images w, w + 16, ...
  objects      compacted into LDS by two waves (rows with cats < 0 are padding, anywhere in the list); M = 0 may come with NULL pointers
  gamma        2 is x * x, anything else powf (the <false> instantiations)

Inputs.  Anchors are synthetic: corners on multiples of 1/8 in [0, 64), widths and heights from SIZES, so that every centre, width and
centre difference of the box encoding is exact in fp32 and the encoding rounds only in its two divisions and the logarithm.  Four fixed
anchors stand in a strip of their own (x < 8; the seeded anchors start at x = 8, and objects derived from them stay right of it): H
(0,0,4,4), F (0,8,5,10) — the one anchor with a width outside SIZES, as the 2/5 construction needs it —, T (0,16,4,20) and S
(0,32,.75,32.75).  An image of kind 'full' (every image of a case with M >= 8 that is not of another kind) holds six fixed objects: (0,0,4,2)
-> IoU exactly 1/2 with H: ignored, not positive; (0,8,2,10) -> fp32(4/10) with F, which is not < fp32(0.4): ignored; T twice with two
categories: the lower row wins; a zero-area box inside H: IoU 0 everywhere; S itself: positive with tw = th = 0.75 clamped to 1.  The other
objects are seeded anchors copied, shifted, stretched (IoU ~0.45) or shrunk by multiples of 1/8.

Tolerances (per element; tolerances() computes them from the fp64 reference alone):
  dclas  |err| <= 1e-5 |ref| + gc 2^-24 |c| (gamma v^(gamma-1) + 2 v^gamma) / u^2     u the logarithm's argument, v the power's base, c =
         alpha or -(1-alpha), gc = g beta / (bs max(npos,1)).  The second term is the one rounding of 1 - raw (<= 2^-25) carried through
         log u and 1/u with a margin of 2: no fp32 evaluation can avoid it, and on the small probabilities of negative anchors it is 2e-4
         of the value, so a plain rtol cannot be used and an absolute floor sized to the tensor would hide exactly those elements.
  dreg   |err| <= 1e-6 |ref| + 2 * 9 gr dt,  dt = 2^-24 (5 + 4 |t|), gr = g (1-beta) / (bs npos 4), t the fp64 target: the encoding's error
         (<= 0.65 dt measured) moves the continuous Huber derivative by at most 9 gr dt.
  out    rtol 2e-5 on out[1], out[2] (non-negative terms, chains under 100 additions) and on out[0]; out[0] also equals
         (1-beta) out[1] + beta out[2] of the kernel's own fp32 values to 2 ulp.
  exact  state, npos; dreg == 0 off the positives; dclas == 0 on ignored anchors and where clas is outside [fp32(1e-4), 1 - fp32(1e-4)],
         != 0 on the two ends of that range.
Measured with restate32() over the whole table (tests/test_retina_cases_cpu.py prints them): worst err / tolerance 0.49 for dclas, 0.14
for dreg, 0.12 for out.  Observed on an MI355X (tests/test_retina_abi_gpu.py, worst over the table): out 0.118, dreg 0.140, dclas 0.487 —
the kernel errs as the numpy restatement does, case by case.
"""
import collections
import functools

import numpy as np
import torch

f32 = np.float32
SENTINEL = 12345.0                               # float outputs are pre-filled with it; no output of these inputs comes near it
STATE_SENTINEL = 0x5A5A5A5A                      # int32 pre-fill of `state`: no object index, not -1, not -2
KBLOCK, KPRE, KMAXOBJ = 256, 8, 128              # retina_loss.hip: anchors per chunk, prefetched pieces per lane, objects per image
SIZES = (0.75, 2.0, 4.0, 8.0, 16.0, 24.0)
LO, HI = f32(1e-4), f32(1) - f32(1e-4)           # the clamp range as the kernel holds it
EXACT_CLAS = (f32(0), f32(1), f32(1e-5), f32(1) - f32(1e-6), LO, HI)
REG_OFFSETS = (0.0, 0.05, -0.05, 1 / 9 - 1e-3, -(1 / 9 - 1e-3), 1 / 9 + 1e-3, -(1 / 9 + 1e-3), 1.0, -1.0)
OUT_RTOL = 2e-5

# the fixed strip (x < 8)
ANCH_H, ANCH_F, ANCH_T, ANCH_S = (0, 0, 4, 4), (0, 8, 5, 10), (0, 16, 4, 20), (0, 32, 0.75, 32.75)
OBJ_HALF, OBJ_TWOFIFTHS, OBJ_ZERO = (0, 0, 4, 2), (0, 8, 2, 10), (2, 2, 2, 3)

Case = collections.namedtuple('Case', 'name bs A K M gamma alpha beta g pad kinds')


def C(name, bs, A, K, M, gamma=2.0, alpha=0.25, beta=0.5, g=1.0, pad='end', kinds=None):
    """pad: where an image's padding rows (cats = -1) go: 'end', 'inter' (between the valid rows, row 0 among them) or 'none';
    kinds: per image, cycled: 'full' (the six fixed objects + derived ones), 'rand' (derived ones only), 'nopos' (objects, but no anchor
    reaches IoU > 0.5), 'allpad' (every row padding), 'null' (M = 0: boxes and cats are NULL)"""
    if kinds is None:
        kinds = ('null',) if M == 0 else ('full',) if M >= 8 else ('rand',)
    return Case(name, bs, A, K, M, gamma, alpha, beta, g, pad, tuple(kinds))


CASES = [
    # scalar class path
    C('k1-a9-m1', 1, 9, 1, 1),
    C('k1-a257-m8-g1', 2, 257, 1, 8, gamma=1.0, alpha=0.6, beta=0.3, g=2.5, pad='inter'),
    C('k3-a257-m8', 2, 257, 3, 8, pad='inter'),
    C('k3-a9-bs33-g15', 33, 9, 3, 3, gamma=1.5, kinds=('rand', 'nopos', 'allpad')),
    C('k21-a700-m64', 2, 700, 21, 64, pad='none'),
    C('k21-a256-g15-beta1', 1, 256, 21, 8, gamma=1.5, alpha=0.6, beta=1.0, pad='inter'),
    # vector class path, every piece prefetched
    C('k4-a256-m8', 1, 256, 4, 8),
    C('k4-a16385', 1, 16385, 4, 8, pad='inter'),
    C('k4-a257-bs17', 17, 257, 4, 8, pad='inter', kinds=('full', 'allpad', 'nopos', 'rand')),
    C('k4-a9-g1-beta0', 2, 9, 4, 2, gamma=1.0, beta=0.0),
    C('k4-a257-bs33', 33, 257, 4, 8, g=2.5, kinds=('full', 'rand', 'allpad')),
    C('k20-a700-m128', 2, 700, 20, 128, pad='inter'),
    C('k20-a257-m0', 2, 257, 20, 0),
    C('k20-a700-m1', 1, 700, 20, 1),
    C('k20-a257-g15', 2, 257, 20, 8, gamma=1.5, alpha=0.6, beta=0.3, g=2.5, pad='inter'),
    C('k20-a256-m64-g1', 1, 256, 20, 64, gamma=1.0, pad='inter'),
    C('k20-a9-bs17', 17, 9, 20, 3, beta=0.3, kinds=('rand', 'allpad', 'nopos')),
    # vector class path with the tail loop
    C('k36-a256-m8', 1, 256, 36, 8, pad='inter'),
    C('k36-a700-m65-g15', 2, 700, 36, 65, gamma=1.5, alpha=0.6, beta=0.3, pad='inter'),
    C('k36-a9-m2', 1, 9, 36, 2),
    C('k80-a257-m65', 2, 257, 80, 65, pad='inter'),
    C('k80-a700-m128-g1', 1, 700, 80, 128, gamma=1.0, g=2.5, pad='inter'),
    C('k80-a256-m0', 1, 256, 80, 0),
    C('k80-a257-beta1', 2, 257, 80, 8, beta=1.0, pad='inter', kinds=('full', 'nopos')),
    C('k36-a257-beta0-g25', 2, 257, 36, 8, beta=0.0, g=2.5, kinds=('full', 'allpad')),
]
CHAINED = ('k3-a257-m8', 'k20-a257-g15', 'k36-a700-m65-g15')            # one per class path: the kernel's own state into its backward
PERMUTED = 'k20-a700-m128'                                               # padding rows moved to the end: every output bitwise equal
ALONE = 'k4-a257-bs17'                                                   # each image alone (bs = 1) against the batch


def case(name):
    return next(c for c in CASES if c.name == name)


def cdiv(a, b):
    return -(-a // b)


def kind_of(c, i):
    return c.kinds[i % len(c.kinds)]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % (2 ** 31)


def make_anchors(A, rs):
    """[A,4] fp32: H, F first, S, T last (T is the last anchor: the one anchor of a tail chunk at A = 257), seeded ones between"""
    n = A - 4
    assert n >= 1
    w, h = (np.array(SIZES)[rs.randint(0, len(SIZES), n)] for _ in range(2))
    x1 = 8 + np.floor(rs.uniform(0, 1, n) * (56 - w) * 8) / 8
    y1 = np.floor(rs.uniform(0, 1, n) * (64 - h) * 8) / 8
    a = np.concatenate([[ANCH_H, ANCH_F], np.stack([x1, y1, x1 + w, y1 + h], 1), [ANCH_S, ANCH_T]]).astype(f32)
    assert a.shape == (A, 4) and (a >= 0).all() and (a < 64).all() and (a * 8 == np.round(a * 8)).all()
    assert ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) > 0).all()
    return a


def _eighths(v):
    return max(0.125, round(v * 8) / 8)


def derive(a, how):
    """an object from a seeded anchor: 0 copy (IoU 1), 1 shift by ~w/8 (and h/8) (positive, centre targets), 2 stretch to IoU ~0.45
    (ignored), 3 shrink to ~3/4 of the width (positive, size targets; below 1 for the 0.75-wide anchors: the tw clamp)"""
    x1, y1, x2, y2 = (float(v) for v in a)
    w, h = x2 - x1, y2 - y1
    if how == 1:
        dx, dy = _eighths(w / 8), (_eighths(h / 8) if w >= 2 and h >= 2 else 0.0)
        return (x1 + dx, y1 + dy, x2 + dx, y2 + dy)
    if how == 2:
        return (x1, y1, x2 + _eighths(1.22 * w), y2)
    if how == 3:
        return (x1, y1, x2 - _eighths(w / 4), y2)
    return (x1, y1, x2, y2)


def _image_objects(c, kind, anchors, rs):
    """(boxes [M,4], cats [M]) of one image, padded with -1"""
    M, K, A = c.M, c.K, c.A
    boxes, cats = -np.ones((M, 4), f32), -np.ones(M, np.int64)
    if kind in ('allpad', 'null') or M == 0:
        return boxes, cats
    n_pad = 0 if c.pad == 'none' else max(1, M // 4) if M > 1 else 0
    n_valid = M - n_pad
    if kind == 'nopos':
        objs = [OBJ_HALF, OBJ_TWOFIFTHS, OBJ_ZERO][:n_valid]
    else:
        objs = []
        if kind == 'full':
            assert n_valid >= 6
            objs = [OBJ_HALF, OBJ_TWOFIFTHS, ANCH_T, ANCH_T, OBJ_ZERO, ANCH_S]
        n_der = n_valid - len(objs)
        src = 2 + rs.permutation(A - 4)[:n_der]                       # distinct seeded anchors
        assert len(src) == n_der, 'too few anchors for %d derived objects' % n_der
        der = [derive(anchors[s], j % 4) for j, s in enumerate(src)]
        if der:
            der[-1] = derive(anchors[src[-1]], 0)                        # the last one is a copy: a positive anchor of its own
        order = rs.permutation(len(objs) + n_der)
        allo = objs + der
        last = allo[-1]
        objs = [allo[j] for j in order if j != len(allo) - 1] + [last]   # shuffled, the guaranteed copy stays the last valid row
    n_valid = len(objs)
    if c.pad == 'inter' and M > n_valid:
        # padding between the valid rows: row 0 is padding, the last row is valid (M = 65: slot 64), the others seeded
        free = 1 + rs.permutation(M - 2)[:M - n_valid - 1] if M > 2 else np.zeros(0, int)
        padrows = set([0] + [int(v) for v in free])
        rows = [r for r in range(M) if r not in padrows][:n_valid]
    else:
        rows = list(range(n_valid))
    ob = np.array(objs, f32).reshape(-1, 4)
    assert (ob * 8 == np.round(ob * 8)).all()
    boxes[rows] = ob
    cc = rs.randint(0, K, n_valid)
    if kind == 'full' and K > 1:                                         # the two T objects carry different categories
        i1, i2 = [j for j, o in enumerate(objs) if tuple(o) == tuple(float(v) for v in ANCH_T)]
        cc[i2] = (cc[i1] + 1) % K
    cats[rows] = cc
    return boxes, cats


def make_clas(shape, rs):
    """the mixture: half uniform inside the clamp range, a fifth log-uniform near each end, a tenth the exact edge values"""
    n = int(np.prod(shape))
    pick = rs.uniform(0, 1, n)
    v = rs.uniform(1e-4, 0.9999, n)
    lo = 10.0 ** rs.uniform(-4, -1, n)
    hi = 1.0 - 10.0 ** rs.uniform(-4, -1, n)
    v = np.where(pick < 0.5, v, np.where(pick < 0.7, lo, hi)).astype(f32)
    ex = np.array(EXACT_CLAS, f32)[rs.randint(0, len(EXACT_CLAS), n)]
    return np.where(pick >= 0.9, ex, v).astype(f32).reshape(shape)


def pad_to_end(boxes, cats):
    """the same images with every padding row moved behind the valid rows, whose order is kept"""
    b2, c2 = -np.ones_like(boxes), -np.ones_like(cats)
    for i in range(len(cats)):
        keep = cats[i] >= 0
        n = int(keep.sum())
        b2[i, :n], c2[i, :n] = boxes[i][keep], cats[i][keep]
    return b2, c2


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = case(name)
    rs = np.random.RandomState(_seed(c))
    anchors = make_anchors(c.A, rs)
    boxes, cats = np.zeros((c.bs, c.M, 4), f32), np.zeros((c.bs, c.M), np.int64)
    for i in range(c.bs):
        boxes[i], cats[i] = _image_objects(c, kind_of(c, i), anchors, rs)
    clas = make_clas((c.bs, c.A, c.K), rs)
    reg = (rs.standard_normal((c.bs, c.A, 4)) * 0.3).astype(f32)
    # a quarter of the positives: reg = the fp32 target + an offset on either side of the Huber knee, on it, or zero
    n = 0
    for i in range(c.bs):
        st = match32(anchors, boxes[i][cats[i] >= 0])
        pos = np.nonzero(st >= 0)[0][::4]
        if len(pos):
            t = encode32(anchors[pos], boxes[i][cats[i] >= 0][st[pos]])
            off = np.array([[REG_OFFSETS[(4 * (n + j) + k) % len(REG_OFFSETS)] for k in range(4)] for j in range(len(pos))])
            reg[i, pos] = (t.astype(np.float64) + off).astype(f32)
            n += len(pos)
    d = dict(anchors=anchors, reg=reg, clas=clas, boxes=boxes, cats=cats)
    for v in d.values():
        v.setflags(write=False)
    return d


def make_inputs(c):
    """{anchors [A,4], reg [bs,A,4], clas [bs,A,K], boxes [bs,M,4], cats [bs,M]} as read-only numpy arrays (shared: do not write)"""
    return _inputs(c.name)


# ---- the state: numpy fp32, the kernel's operations in the kernel's order -------------------------------------------------------------------
def match32(anchors, objs):
    """state int32 [A] of one image from its valid objects [m,4] (fp32 throughout)"""
    A = len(anchors)
    if len(objs) == 0:
        return np.full(A, -1, np.int32)
    a, o = anchors.astype(f32), objs.astype(f32)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_o = (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1])
    iw = np.maximum(np.minimum(o[:, None, 2], a[None, :, 2]) - np.maximum(o[:, None, 0], a[None, :, 0]), f32(0))
    ih = np.maximum(np.minimum(o[:, None, 3], a[None, :, 3]) - np.maximum(o[:, None, 1], a[None, :, 1]), f32(0))
    inter = iw * ih
    iou = inter / ((area_o[:, None] + area_a[None, :]) - inter)
    assert iou.dtype == f32 and not np.isnan(iou).any()
    arg = iou.argmax(0)                                                  # the first maximum
    best = iou.max(0)
    st = np.full(A, -2, np.int32)
    st[best < f32(0.4)] = -1
    pos = best > f32(0.5)
    st[pos] = arg[pos]
    return st


def iou32(anchor, obj):
    a, o = np.array(anchor, f32), np.array(obj, f32)
    iw = max(min(o[2], a[2]) - max(o[0], a[0]), f32(0))
    ih = max(min(o[3], a[3]) - max(o[1], a[1]), f32(0))
    inter = f32(iw * ih)
    return f32(inter / f32(f32((o[2] - o[0]) * (o[3] - o[1]) + (a[2] - a[0]) * (a[3] - a[1])) - inter))


def encode32(a, o):
    """targets [n,4] in fp32 (restatement of encode_box)"""
    a, o = a.astype(f32), o.astype(f32)
    aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    acx, acy = a[:, 0] + f32(0.5) * aw, a[:, 1] + f32(0.5) * ah
    tw, th = o[:, 2] - o[:, 0], o[:, 3] - o[:, 1]
    tcx, tcy = o[:, 0] + f32(0.5) * tw, o[:, 1] + f32(0.5) * th
    tw, th = np.maximum(tw, f32(1)), np.maximum(th, f32(1))
    t = np.stack([((tcx - acx) / aw) / f32(0.1), ((tcy - acy) / ah) / f32(0.1), np.log(tw / aw) / f32(0.2), np.log(th / ah) / f32(0.2)], 1)
    assert t.dtype == f32
    return t


def encode64(a, o):
    """targets [n,4] in torch fp64 from fp32 boxes cast up; 0.1 and 0.2 as their fp32 values"""
    aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    acx, acy = a[:, 0] + 0.5 * aw, a[:, 1] + 0.5 * ah
    tw, th = o[:, 2] - o[:, 0], o[:, 3] - o[:, 1]
    tcx, tcy = o[:, 0] + 0.5 * tw, o[:, 1] + 0.5 * th
    tw, th = tw.clamp(min=1), th.clamp(min=1)
    c1, c2 = float(f32(0.1)), float(f32(0.2))
    return torch.stack([((tcx - acx) / aw) / c1, ((tcy - acy) / ah) / c1, torch.log(tw / aw) / c2, torch.log(th / ah) / c2], 1)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def reference_of(anchors, reg, clas, boxes, cats, beta, alpha, gamma, g):
    """state / npos (fp32 restatement, exact) and out, per-image terms, dreg, dclas (torch fp64 autograd, given that state) of numpy fp32
    inputs; the hyper-parameters as the fp32 values the ABI passes.  Returns numpy arrays plus the per-element tolerances."""
    bs, A, K = clas.shape
    beta, alpha, gamma, g = (float(f32(v)) for v in (beta, alpha, gamma, g))
    lo, hi = float(LO), float(HI)
    a64 = torch.from_numpy(np.array(anchors, np.float64))
    r64 = torch.from_numpy(np.array(reg, np.float64)).requires_grad_(True)
    c64 = torch.from_numpy(np.array(clas, np.float64)).requires_grad_(True)
    state = np.zeros((bs, A), np.int32)
    tcls = np.full((bs, A), -1, np.int64)                             # target class of a positive anchor
    target = np.zeros((bs, A, 4))
    img_reg, img_clas = [], []
    for i in range(bs):
        keep = cats[i] >= 0 if cats is not None and cats.shape[1] else np.zeros(0, bool)
        objs = boxes[i][keep] if keep.any() else np.zeros((0, 4), f32)
        st = match32(anchors, objs)
        state[i] = st
        pos = np.nonzero(st >= 0)[0]
        used = torch.from_numpy(st != -2)
        if len(pos):
            tcls[i, pos] = cats[i][keep][st[pos]]
        onehot = torch.zeros(A, K, dtype=torch.bool)
        onehot[torch.from_numpy(pos), torch.from_numpy(tcls[i, pos])] = True
        p = c64[i].clamp(lo, hi)
        term = torch.where(onehot, -alpha * (1 - p).pow(gamma) * torch.log(p), -(1 - alpha) * p.pow(gamma) * torch.log(1 - p))
        img_clas.append(term[used].sum() / max(len(pos), 1))
        if len(pos):
            t = encode64(a64[pos], torch.from_numpy(np.array(objs, np.float64))[st[pos]])
            target[i, pos] = t.numpy()
            d = (t - r64[i][pos]).abs()
            img_reg.append(torch.where(d < 1 / 9, 4.5 * d * d, d - 0.5 / 9).sum() / (len(pos) * 4))
        else:
            img_reg.append(torch.zeros((), dtype=torch.float64))
    reg_loss, clas_loss = torch.stack(img_reg).sum() / bs, torch.stack(img_clas).sum() / bs
    total = (1 - beta) * reg_loss + beta * clas_loss
    (total * g).backward()
    npos = (state >= 0).sum(1).astype(f32)
    r = dict(state=state, npos=npos, tcls=tcls, target=target, clas=clas,
             out=np.array([total.item(), reg_loss.item(), clas_loss.item()]),
             img_reg=torch.stack(img_reg).detach().numpy(), img_clas=torch.stack(img_clas).detach().numpy(),
             dreg=np.zeros(reg.shape) if r64.grad is None else r64.grad.numpy(), dclas=c64.grad.numpy())
    r.update(tolerances(clas, r, beta, alpha, gamma, g))
    return r


def tolerances(clas, r, beta, alpha, gamma, g):
    """the per-element bounds of the module docstring, from the fp64 reference alone.  beta, alpha, gamma, g: fp32 values as floats"""
    bs, A, K = clas.shape
    n = r['npos'].astype(np.float64)
    raw = clas.astype(np.float64)
    is_t = np.zeros((bs, A, K), bool)
    bi, ai = np.nonzero(r['tcls'] >= 0)
    is_t[bi, ai, r['tcls'][bi, ai]] = True
    inside = (clas >= LO) & (clas <= HI)
    live = inside & (r['state'] != -2)[:, :, None]                    # where a gradient flows
    u = np.where(is_t, raw, 1 - raw)
    v = np.where(is_t, 1 - raw, raw)
    cabs = np.where(is_t, alpha, 1 - alpha)
    gc = (g * beta / (bs * np.maximum(n, 1)))[:, None, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        intrinsic = gc * 2.0 ** -24 * cabs * (gamma * v ** (gamma - 1) + 2 * v ** gamma) / u ** 2
    tol_dclas = np.where(live, 1e-5 * np.abs(r['dclas']) + np.where(live, intrinsic, 0), 0.0)
    gr = np.where(n > 0, g * (1 - beta) / (bs * np.maximum(n, 1) * 4), 0.0)[:, None, None]
    dt = 2.0 ** -24 * (5 + 4 * np.abs(r['target']))
    tol_dreg = np.where((r['state'] >= 0)[:, :, None], 1e-6 * np.abs(r['dreg']) + 2 * 9 * gr * dt, 0.0)
    return dict(is_target=is_t, inside=inside, live=live, tol_dclas=tol_dclas, tol_dreg=tol_dreg, dt=dt)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = case(name)
    d = make_inputs(c)
    return reference_of(d['anchors'], d['reg'], d['clas'], d['boxes'], d['cats'], c.beta, c.alpha, c.gamma, c.g)


def reference(c):
    """computed once per case and shared: do not write to it"""
    return _reference(c.name)


# ---- the same arithmetic in numpy fp32: validates the tolerances, judges nothing ----------------------------------------------------------------
def restate32(c, d, r):
    """out, dreg, dclas as a correct fp32 evaluation gives them (focal_term / focal_grad / encode_box / the Huber branches of
    retina_loss.hip, each operation rounded to fp32; the sums pairwise), from the reference's state"""
    bs, A, K = d['clas'].shape
    alpha, beta, gamma, g = f32(c.alpha), f32(c.beta), f32(c.gamma), f32(c.g)
    one = f32(1)
    raw = d['clas']
    is_t, st = r['is_target'], r['state']
    used = (st != -2)[:, :, None]
    # forward
    p = np.minimum(np.maximum(raw, LO), HI)
    q = one - p
    w = np.where(is_t, alpha * np.power(q, gamma), (one - alpha) * np.power(one - q, gamma))
    term = np.where(used, -w * np.log(np.where(is_t, p, q)), f32(0))
    assert term.dtype == f32
    # focal gradient
    u, v = np.where(is_t, raw, one - raw), np.where(is_t, one - raw, raw)
    cc = np.where(is_t, alpha, -(one - alpha)).astype(f32)
    with np.errstate(divide='ignore', invalid='ignore'):
        dd = cc * (gamma * np.power(v, gamma - one) * np.log(u) - np.power(v, gamma) / u)
        n = r['npos']
        gc = (g * beta / (f32(bs) * np.maximum(n, one))).astype(f32)[:, None, None]
        dclas = np.where(r['inside'] & used, dd * gc, f32(0)).astype(f32)
    gr = np.where(n > 0, g * (one - beta) / (f32(bs) * np.maximum(n, one) * f32(4)), f32(0)).astype(f32)
    dreg = np.zeros((bs, A, 4), f32)
    clas_sum, reg_sum = f32(0), f32(0)
    for i in range(bs):
        keep = d['cats'][i] >= 0 if c.M else np.zeros(0, bool)
        pos = np.nonzero(st[i] >= 0)[0]
        clas_sum += term[i].sum(dtype=f32) / max(n[i], one)
        if len(pos):
            t = encode32(d['anchors'][pos], d['boxes'][i][keep][st[i][pos]])
            diff = t - d['reg'][i][pos]
            ad = np.abs(diff)
            knee = one / f32(9)
            reg_sum += np.where(ad < knee, f32(4.5) * (ad * ad), ad - f32(0.5) / f32(9)).sum(dtype=f32) / (n[i] * f32(4))
            dreg[i, pos] = -np.sign(diff) * np.where(ad < knee, f32(9) * ad, one) * gr[i]
    cl, rg = f32(clas_sum / f32(bs)), f32(reg_sum / f32(bs))
    out = np.array([(one - beta) * rg + beta * cl, rg, cl], f32)
    assert dclas.dtype == f32 and dreg.dtype == f32
    return dict(out=out, dreg=dreg, dclas=dclas)


# ---- the checks (what the GPU test applies to the kernel, and the CPU test to restate32) -----------------------------------------------------
def _ratio(err, tol):
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def check_forward(c, r, state, npos, out, what=''):
    """state and npos exactly, out within OUT_RTOL of fp64 and out[0] the combination of the kernel's own two terms; returns the worst
    err / tolerance of out"""
    ctx = '%s%s' % (c.name, what)
    state, npos, out = np.asarray(state), np.asarray(npos), np.asarray(out)
    assert state.dtype == np.int32 and state.shape == r['state'].shape
    bad = np.argwhere(state != r['state'])
    assert len(bad) == 0, '%s: state differs at %d anchors, first (image, anchor) %s: got %d, reference %d' % (
        ctx, len(bad), bad[0], state[tuple(bad[0])], r['state'][tuple(bad[0])])
    assert np.array_equal(npos, r['npos']), '%s: npos %s, reference %s' % (ctx, npos, r['npos'])
    assert out.dtype == f32 and out.shape == (3,) and np.isfinite(out).all(), '%s: out %s' % (ctx, out)
    err, tol = np.abs(out.astype(np.float64) - r['out']), OUT_RTOL * np.abs(r['out'])
    assert (err <= tol).all(), '%s: out %s, fp64 %s: err / tol %s' % (ctx, out, r['out'], err / np.maximum(tol, 1e-300))
    beta = f32(c.beta)
    own = f32(f32((f32(1) - beta) * out[1]) + f32(beta * out[2]))
    assert abs(float(out[0]) - float(own)) <= 2 * float(np.spacing(np.abs(own))), '%s: out[0] %r is not (1-beta) out[1] + beta out[2] = %r' % (
        ctx, out[0], own)
    return _ratio(err, tol)


def check_backward(c, r, dreg, dclas, what=''):
    """the exact zeros, the nonzero ends of the clamp range and the per-element tolerances; returns (worst dreg ratio, worst dclas ratio)"""
    ctx = '%s%s' % (c.name, what)
    dreg, dclas = np.asarray(dreg), np.asarray(dclas)
    assert dreg.dtype == f32 and dclas.dtype == f32 and dreg.shape == r['dreg'].shape and dclas.shape == r['dclas'].shape
    assert np.isfinite(dreg).all() and np.isfinite(dclas).all(), '%s: a gradient is not finite' % ctx
    clas = r['clas']
    nonpos = (r['state'] < 0)[:, :, None]
    assert not (dreg != 0)[np.broadcast_to(nonpos, dreg.shape)].any(), '%s: dreg is not exactly 0 on an anchor that is not positive' % ctx
    assert not (dclas != 0)[~r['live']].any(), '%s: dclas is not exactly 0 on an ignored anchor or outside the clamp range: %d elements' % (
        ctx, int((dclas != 0)[~r['live']].sum()))
    if c.beta != 0:
        ends = r['live'] & ((clas == LO) | (clas == HI))
        assert (dclas != 0)[ends].all(), '%s: dclas is 0 on an end of the clamp range (the clamp passes the gradient there)' % ctx
    e_r, e_c = np.abs(dreg.astype(np.float64) - r['dreg']), np.abs(dclas.astype(np.float64) - r['dclas'])
    q_r, q_c = _ratio(e_r, r['tol_dreg']), _ratio(e_c, r['tol_dclas'])
    if q_r > 1:
        i = np.unravel_index(np.argmax(e_r - r['tol_dreg']), e_r.shape)
        raise AssertionError('%s: dreg %s: got %r, fp64 %r, err %.3e, tolerance %.3e (worst ratio %.2f)' % (
            ctx, i, dreg[i], r['dreg'][i], e_r[i], r['tol_dreg'][i], q_r))
    if q_c > 1:
        i = np.unravel_index(np.argmax(e_c - r['tol_dclas']), e_c.shape)
        raise AssertionError('%s: dclas %s (clas %r, target class %s, state %d): got %r, fp64 %r, err %.3e, tolerance %.3e (worst ratio %.2f)' % (
            ctx, i, clas[i], bool(r['is_target'][i]), r['state'][i[0], i[1]], dclas[i], r['dclas'][i], e_c[i], r['tol_dclas'][i], q_c))
    return q_r, q_c


# ---- regimes: named predicates over (case, inputs, reference) -----------------------------------------------------------------------------------
def _pieces(c):
    return min(KBLOCK, c.A) * c.K // 4


def _valid(d, i):
    return d['cats'][i] >= 0


def _m128_both_sides(c, d, r):
    if c.M != 128:
        return False
    for i in range(c.bs):
        v = _valid(d, i)
        first_half = int(v[:64].sum())
        # a compacted index >= the first half's count belongs to a row of the second half (wave 1 of load_objects)
        if v[:64].any() and v[64:].any() and (r['state'][i] >= first_half).any():
            return True
    return False


def _hyper(name, val):
    return lambda c, d, r: abs(getattr(c, name) - val) < 1e-9


REGIMES = collections.OrderedDict([
    ('class scalar K=1', lambda c, d, r: c.K == 1),
    ('class scalar K=3', lambda c, d, r: c.K == 3),
    ('class scalar K=21', lambda c, d, r: c.K == 21),
    ('class vector prefetched K=4', lambda c, d, r: c.K == 4 and _pieces(c) <= KPRE * KBLOCK),
    ('class vector prefetched K=20', lambda c, d, r: c.K == 20 and _pieces(c) <= KPRE * KBLOCK),
    ('class vector tail K=36 full chunk', lambda c, d, r: c.K == 36 and c.A >= KBLOCK and _pieces(c) - KPRE * KBLOCK == 256),
    ('class vector tail K=80', lambda c, d, r: c.K == 80 and _pieces(c) > KPRE * KBLOCK),
    ('class powf scalar', lambda c, d, r: c.gamma != 2 and c.K % 4 != 0),
    ('class powf vector prefetched', lambda c, d, r: c.gamma != 2 and c.K % 4 == 0 and _pieces(c) <= KPRE * KBLOCK),
    ('class powf vector tail', lambda c, d, r: c.gamma != 2 and c.K % 4 == 0 and _pieces(c) > KPRE * KBLOCK),
    ('chunks A=9', lambda c, d, r: c.A == 9),
    ('chunks A=256', lambda c, d, r: c.A == 256),
    ('chunks A=257 tail of one', lambda c, d, r: c.A == 257),
    ('chunks A=700', lambda c, d, r: c.A == 700),
    ('chunks more than 64 (A=16385, K=4, bs=1)', lambda c, d, r: c.A == 16385 and c.K == 4 and c.bs == 1 and cdiv(c.A, KBLOCK) > 64),
    ('batch 1', lambda c, d, r: c.bs == 1),
    ('batch 2', lambda c, d, r: c.bs == 2),
    ('batch 17', lambda c, d, r: c.bs == 17),
    ('batch 33', lambda c, d, r: c.bs == 33),
    ('objects M=0 NULL', lambda c, d, r: c.M == 0),
    ('objects M=1', lambda c, d, r: c.M == 1 and (r['state'] >= 0).any()),
    ('objects M=8 padding between valid rows', lambda c, d, r: c.M == 8 and any(
        (~_valid(d, i))[:np.nonzero(_valid(d, i))[0].max()].any() for i in range(c.bs) if _valid(d, i).any())),
    ('objects M=64', lambda c, d, r: c.M == 64 and _valid(d, 0)[63]),
    ('objects M=65 slot 64 valid', lambda c, d, r: c.M == 65 and all(_valid(d, i)[64] for i in range(c.bs))),
    ('objects M=128 both halves, positive from the second', _m128_both_sides),
    ('objects image all padding', lambda c, d, r: c.M > 0 and any(not _valid(d, i).any() for i in range(c.bs))),
    ('objects image without a positive', lambda c, d, r: any(_valid(d, i).any() and r['npos'][i] == 0 for i in range(c.bs))),
    ('gamma 2', _hyper('gamma', 2.0)), ('gamma 1.5', _hyper('gamma', 1.5)), ('gamma 1', _hyper('gamma', 1.0)),
    ('alpha 0.25', _hyper('alpha', 0.25)), ('alpha 0.6', _hyper('alpha', 0.6)),
    ('beta 0.5', _hyper('beta', 0.5)), ('beta 0.3', _hyper('beta', 0.3)), ('beta 0', _hyper('beta', 0.0)), ('beta 1', _hyper('beta', 1.0)),
    ('upstream 1', _hyper('g', 1.0)), ('upstream 2.5', _hyper('g', 2.5)),
])


def coverage():
    """{regime: [names of the cases that reach it]}"""
    cov = collections.OrderedDict((k, []) for k in REGIMES)
    for c in CASES:
        d, r = make_inputs(c), reference(c)
        for k, pred in REGIMES.items():
            if pred(c, d, r):
                cov[k].append(c.name)
    return cov
