"""The case tables of the detection-INFERENCE C-ABI sweep (tests/test_detect_abi_gpu.py, tests/test_detect_cases_cpu.py), their inputs, their
references, their conditions and the one tolerance.

A plain module: no fixtures, nothing from the library, nothing from the GPU.  It restates the contracts of nnl_bbox_decode,
nnl_bbox_decode_window, nnl_nms and nnl_tta_bbox_merge (include/nnl.h, csrc/detect.hip) as

  decode_ref   numpy fp64 of the fp32 inputs: first maximum of the K scores (a NaN drops the anchor), score > thresh (strict), the box
               cx + w (reg0 std0 + mean0), ..., w exp(reg2 std2 + mean2), ..., clipped to the window, dropped unless both clipped extents
               are > 0; the candidates of an image in anchor order.
  nms_ref      the plain greedy loop in fp64: a stable sort by (score descending, order ascending; the position when order is None), the cut at
               top_k, then in that order a box is kept unless an earlier KEPT box of its class has IoU > max_overlap.
  merge_ref    nnl_tta_bbox_merge in numpy fp32 (the inputs are on a grid where every operation is exact), fillers included.
  restate32()  decode and NMS once more in numpy fp32 with the kernel's operation order (inter / ((a1 + a2) - inter), one rounding per
               operation: the library is built with -ffp-contract=off).  It is no reference: the CPU test runs it through check_decode /
               check_nms to prove that a correct fp32 evaluation passes every check, before any kernel is judged by them.

Launch regimes of csrc/detect.hip the tables are built around (REGIMES holds the predicates; coverage() lists the cases of each):
  decode   256 anchors per block; first maximum; strict thresh; NaN; empty boxes after clipping; the window; per-image counts 0 and A
  rank     256 candidates per block, LDS tiles of 1024 keys; total order (score desc, order asc); the cut at top_k inside a group of equal
           scores; order permuted, order NULL; count 0, count == cap, count above cap (read as cap); -0.0 and +0.0 are one score
  scan     64 boxes per mask word and scan chunk; survivors m of the cut on either side of 64, 128, 192; m == top_k with top_k % 64 != 0;
           suppression carried across chunks through removed[]; a removed box suppresses nothing; same class only; strict IoU compare; 0/0

Two data modes.
  grid    every outcome is exact in fp32: anchor corners and sizes are multiples of 1/8, std = (1/8, 1/8, 1/2, 1/2) and mean =
          (1/4, -1/4, 1/4, 1/4) with reg0, reg1 integers and reg2 = reg3 = -1/2, so that dx, dy are multiples of 1/8 and dw = dh = 0 exactly
          (expf(0) = 1); scores come from GRID_SCORES (thresh itself and the next fp32 above it among them); NMS boxes lie on an integer grid.
          Boxes, classes, scores and counts must match the reference BIT FOR BIT.
  randn   random anchors, reg, clas and boxes against fp64, under CONDITIONS that the reference alone must meet (assert_conditions; the seeds
          are searched so that it does): no two candidates of an image share a score; no best class score within 1e-6 relative of thresh;
          no same-class pair of the ranked top_k with an fp64 IoU within 1e-4 of max_overlap; no candidate whose clipped extent lies within
          1e-3 of 0 (kept or dropped); |dw|, |dh| <= 1.5.  These are conditions, not tolerances: with them the kept set, its order, classes
          and scores are compared exactly, and only decoded box coordinates get a bound.

The box coordinate bound (randn decode), per element, u = 2^-24, counted rounding by rounding along x0 = (cx + w dx) - 0.5 (w e^dw):
  w = a2 - a0 (u w), cx = a0 + 0.5 w (u |cx| for the sum, and the 0.5 u w that w brings along: NOT relative to cx, which may be near 0 while w
  is large; with |dw| <= 1.5 that is at most 0.5 e^1.5 u pw = 2.24 u pw), dx = r0 s0 + m0 with m0 = 0 in the randn cases (rel. u), w dx (rel. u on
  top of those of w and dx: 3 u |w dx|), the sum pcx (u (|cx| + |w dx|)), dw = r2 s2 (|dw| u, which e^dw turns into a relative |dw| u <= 1.5
  u), expf (the device library states 1 ulp <= 2 u relative), w e^dw (rel. u on top of w's u), 0.5 pw exact, and the final difference
  (u (|cx| + |w dx| + 0.5 pw)).  The sum is u (3 |cx| + 5 |w dx| + (2.24 + 0.5 (1 + 1.5 + 2 + 1) + 0.5) pw) = u (3 |cx| + 5 |w dx| + 5.49 pw);
  with a margin,
      bound = u * (A_AFF * (|cx| + |w dx|) + B_EXP * pw),   A_AFF = 6, B_EXP = 6        (the same with cy, h, dy, ph for the y coordinates),
  evaluated on the fp64 reference's values.  Clipping is 1-Lipschitz and moves no error.  On the 128-pixel images of the table the largest
  bound is 7.0e-5 (test_detect_cases_cpu.py asserts it stays under what test_bbox_inference.py grants at that scale, 1e-5 * 128 + 1e-5 =
  1.29e-3).
Measured with restate32() over the whole table (tests/test_detect_cases_cpu.py prints it): worst err / bound 0.402 (r-a2100-k5; 0.307, 0.311
and 0.318 on the other three randn cases), so the restatement sits inside HALF the bound as required.  Observed on an MI355X
(tests/test_detect_abi_gpu.py, worst over the table): 0.402, and 0.307, 0.311, 0.318 — the kernel errs as the numpy restatement does, case by
case; the kept boxes of decode into NMS at most 0.311.  Every grid case matched bit for bit.
"""
import collections
import functools

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
A_AFF, B_EXP = 6, 6
KERNEL_WORST_RATIO = 0.402                       # worst |kernel - fp64| / bound observed on an MI355X over the randn decode cases
SENTINEL = 12345.0                               # float outputs are pre-filled with it; no output of these inputs comes near it
INT_SENTINEL = 0x5A5A5A5A                        # int32 pre-fill: no class, no anchor index, no count
KDECODE, KRANKTILE, KCHUNK = 256, 1024, 64                       # detect.hip: anchors per block, LDS keys per tile, boxes per mask word
IMG = 128.0                                      # decode cases: the image is [0, 128] x [0, 128]
GRID_STD, GRID_MEAN = (0.125, 0.125, 0.5, 0.5), (0.25, -0.25, 0.25, 0.25)
RAND_STD, RAND_MEAN = (0.1, 0.1, 0.2, 0.2), (0.0, 0.0, 0.0, 0.0)
GRID_THRESH = f32(0.25)
ABOVE_THRESH = np.nextafter(GRID_THRESH, f32(1))
GRID_SCORES = (f32(0), f32(0.125), GRID_THRESH, ABOVE_THRESH, f32(0.5), f32(0.75))
HALF, BELOW_HALF = f32(0.5), np.nextafter(f32(0.5), f32(0))
# the fixed anchors of a grid case with edges (the LAST len(EDGE_ANCHORS) anchors; their reg gives dx = dy = 0): wholly outside; zero width
# after clipping at the lower and at the upper bound; zero height at the lower bound; one that the image keeps and the inner window drops
EDGE_ANCHORS = ((-40, -40, -30, -30), (-8, 16, 0, 32), (128, 8, 136, 24), (40, -4, 48, 0), (2, 2, 10, 6), (140, 30, 150, 40))
INNER_WINDOW = (16.0, 8.0, 100.0, 90.0)

DCase = collections.namedtuple('DCase', 'name mode bs A K thresh window kinds edges top_k max_overlap')
NCase = collections.namedtuple('NCase', 'name mode top_k max_overlap images null_order cap')


def D(name, mode, bs, A, K, window=None, kinds=('mixed',), edges=False, top_k=100, max_overlap=0.5, thresh=None):
    """kinds, per image, cycled: 'mixed', 'none' (no score above thresh: zero candidates), 'all' (every anchor is a candidate: count == A; the
    anchors of such a case all lie inside the image)"""
    if thresh is None:
        thresh = float(GRID_THRESH) if mode == 'grid' else 0.4
    return DCase(name, mode, bs, A, K, thresh, window, tuple(kinds), edges, top_k, max_overlap)


DECODE_CASES = [
    D('g-a200-k1', 'grid', 1, 200, 1),
    D('g-a256-k3-bs3', 'grid', 3, 256, 3, kinds=('mixed', 'none', 'all'), top_k=64),
    D('g-a257-k4-edges', 'grid', 2, 257, 4, edges=True, top_k=200),
    D('g-a700-k2-window', 'grid', 2, 700, 2, window=INNER_WINDOW, edges=True, top_k=129),
    D('g-a513-k3-whole', 'grid', 1, 513, 3, window=(0.0, 0.0, IMG, IMG), edges=True, top_k=260),
    D('r-a257-k1-bs3', 'randn', 3, 257, 1, kinds=('mixed', 'none', 'mixed'), top_k=64),
    D('r-a300-k7-window', 'randn', 2, 300, 7, window=INNER_WINDOW, top_k=100, max_overlap=0.4),
    D('r-a512-k20', 'randn', 1, 512, 20, top_k=200, thresh=0.8),
    D('r-a2100-k5', 'randn', 2, 2100, 5, top_k=260),
]
WHOLE_WINDOW = 'g-a513-k3-whole'                 # a window equal to the image: bitwise what nnl_bbox_decode gives


def N(name, top_k, images, max_overlap=HALF, mode='grid', null_order=False, cap=None):
    """images: one spec per image, (kind, n, ...): see _image"""
    return NCase(name, mode, top_k, float(f32(max_overlap)), tuple(images), null_order, cap)


NMS_CASES = [
    # rank-sort: disjoint boxes (everything ranked is kept), groups of equal scores, order permuted against position
    N('rank-n0', 64, [('rank', 0)]),
    N('rank-n1', 64, [('rank', 1)]),
    N('rank-n255-k300', 300, [('rank', 255)]),
    N('rank-n256-k256', 256, [('rank', 256)]),
    N('rank-n257-k100', 100, [('rank', 257)]),
    N('rank-n1023-k200', 200, [('rank', 1023)]),
    N('rank-n1024-k64', 64, [('rank', 1024)]),
    N('rank-n1025-k129', 129, [('rank', 1025)]),
    N('rank-n2100-k260', 260, [('rank', 2100)]),
    N('rank-n257-null', 100, [('rank', 257)], null_order=True),
    N('rank-n1025-null', 193, [('rank', 1025)], null_order=True),
    N('rank-batch', 100, [('rank', 0), ('rank', 300), ('rank', 63), ('rank', 300, 'over'), ('rank', 100)]),
    N('rank-signed-zero', 3, [('signed_zero', 6)]),
    # mask and scan
    N('scan-same-m200', 200, [('same', 230)]),
    N('scan-classes-m65', 100, [('classes', 65)]),
    N('scan-pairs-k100', 100, [('pairs', 200)]),
    N('scan-chain-across-1', 200, [('chain', 150, (10, 70, 75))]),
    N('scan-chain-across-2', 200, [('chain', 200, (63, 64, 128))]),
    N('scan-chain-inside', 64, [('chain', 63, (10, 20, 30))]),
    N('scan-iou-equal', 64, [('iou_eq', 5)], max_overlap=HALF),
    N('scan-iou-below', 64, [('iou_eq', 5)], max_overlap=BELOW_HALF),
    N('scan-zero-area', 64, [('zero_area', 8)]),
    N('scan-rand-n300-k200', 200, [('rand', 300), ('rand', 64), ('rand', 0), ('rand', 129)], mode='randn'),
    N('scan-rand-n1025-k260', 260, [('rand', 1025), ('rand', 128)], mode='randn', max_overlap=0.3),
    N('scan-rand-n257-k100', 100, [('rand', 257), ('rand', 1), ('rand', 65)], mode='randn', max_overlap=0.6),
    N('scan-rand-n500-k193', 193, [('rand', 500), ('rand', 63)], mode='randn', null_order=True),
]
SHUFFLED = ('rank-n1025-k129', 'rank-n2100-k260', 'scan-rand-n300-k200', 'scan-chain-across-2')   # storage order permuted: bitwise equal outputs
MERGE_P = (1, 64)


def dcase(name):
    return next(c for c in DECODE_CASES if c.name == name)


def ncase(name):
    return next(c for c in NMS_CASES if c.name == name)


def cdiv(a, b):
    return -(-a // b)


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def kind_of(c, i):
    return c.kinds[i % len(c.kinds)]


def window_of(c):
    return (0.0, 0.0, IMG, IMG) if c.window is None else c.window


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- decode: inputs --------------------------------------------------------------------------------------------------------------------------
def _grid_decode_inputs(c, rs):
    A, K, ne = c.A, c.K, len(EDGE_ANCHORS) if c.edges else 0
    n = A - ne
    sizes = np.array((2.0, 4.0, 8.0, 16.0, 32.0))
    w, h = sizes[rs.randint(0, 5, n)], sizes[rs.randint(0, 5, n)]
    inside = 'all' in c.kinds
    lo, hi = (8.0, 88.0) if inside else (-16.0, 128.0)
    x0, y0 = (np.floor(rs.uniform(lo, hi, n) * 8) / 8 for _ in range(2))
    anchors = np.stack([x0, y0, x0 + w, y0 + h], 1)
    if ne:
        anchors = np.concatenate([anchors, np.array(EDGE_ANCHORS, f64)])
    reg = np.zeros((c.bs, A, 4))
    reg[:, :, 0], reg[:, :, 1] = rs.randint(-6, 3, (c.bs, A)), rs.randint(-2, 7, (c.bs, A))      # dx, dy in [-1/2, 1/2], multiples of 1/8
    reg[:, :, 2:] = -0.5                                                                         # dw = dh = -1/2 * 1/2 + 1/4 = 0
    if ne:
        reg[:, n:, 0], reg[:, n:, 1] = -2.0, 2.0                                                 # dx = dy = 0: the edge anchors stay put
    clas = np.zeros((c.bs, A, K), f32)
    for i in range(c.bs):
        pool = {'mixed': GRID_SCORES, 'none': GRID_SCORES[:3], 'all': GRID_SCORES[3:]}[kind_of(c, i)]
        clas[i] = np.array(pool, f32)[rs.randint(0, len(pool), (A, K))]
        if kind_of(c, i) == 'mixed':
            if ne:
                clas[i, n:, :] = f32(0.125)
                clas[i, n:, K - 1] = f32(0.75)                        # the edge anchors pass the threshold: the clipping decides
            if c.edges:                                              # NaN rows: among scores above thresh, in the first / a middle / the last class
                rows = rs.permutation(n)[:9]
                for j, a in enumerate(rows):
                    clas[i, a] = f32(0.75) if j % 3 else f32(0.5)
                    clas[i, a, (0, K // 2, K - 1)[j % 3]] = np.nan
    return dict(anchors=anchors.astype(f32), reg=reg.astype(f32), clas=clas, mean=np.array(GRID_MEAN, f32), std=np.array(GRID_STD, f32))


def _rand_decode_inputs(c, rs):
    A, K = c.A, c.K
    w, h = rs.uniform(6, 40, A), rs.uniform(6, 40, A)
    cx, cy = rs.uniform(-4, IMG + 4, A), rs.uniform(-4, IMG + 4, A)
    anchors = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(f32)
    reg = rs.standard_normal((c.bs, A, 4)).astype(f32)
    clas = rs.uniform(0, 1, (c.bs, A, K)).astype(f32)
    for i in range(c.bs):
        if kind_of(c, i) == 'none':
            clas[i] *= f32(c.thresh * 0.9)
    return dict(anchors=anchors, reg=reg, clas=clas, mean=np.array(RAND_MEAN, f32), std=np.array(RAND_STD, f32))


@functools.lru_cache(maxsize=None)
def _decode_inputs(name):
    c = dcase(name)
    for attempt in range(64):                                         # randn: the first seed whose REFERENCE meets the conditions
        rs = np.random.RandomState(_seed(name) + attempt)
        d = _grid_decode_inputs(c, rs) if c.mode == 'grid' else _rand_decode_inputs(c, rs)
        if c.mode == 'grid' or not decode_condition_failures(c, d):
            d['attempt'] = attempt
            return _frozen(d)
    raise AssertionError('%s: no seed meets the conditions' % name)


def decode_inputs(c):
    """{anchors [A,4], reg [bs,A,4], clas [bs,A,K], mean [4], std [4]} read-only fp32 arrays (shared: do not write)"""
    return _decode_inputs(c.name)


# ---- decode: one arithmetic for the reference (fp64), the restatement (fp32) and the mutants ----------------------------------------------------
def _decode(c, d, dt, mutant=None):
    """per image a dict of the candidates in anchor order: order [n], classes [n] i32, scores [n] f32 (copies), boxes [n,4] dt, bound [n,4],
    extent [n',2] (clipped extents of every anchor above thresh, dropped ones included), best [A] (nan where a score is NaN)"""
    an, mean, std = d['anchors'].astype(dt), d['mean'].astype(dt), d['std'].astype(dt)
    xlo, ylo, xhi, yhi = (dt(v) for v in window_of(c))
    if mutant == 'window_lo_ignored':
        xlo = ylo = dt(0)
    half = dt(0.5)
    out = []
    for i in range(c.bs):
        clas, r = d['clas'][i], d['reg'][i].astype(dt)
        nan = np.isnan(clas).any(1)
        safe = np.where(np.isnan(clas), f32(-np.inf), clas)
        bk = safe.argmax(1) if mutant != 'last_max' else c.K - 1 - safe[:, ::-1].argmax(1)
        best = np.where(nan, f32(np.nan), safe[np.arange(c.A), bk]).astype(f32)
        with np.errstate(invalid='ignore'):
            hit = (best >= f32(c.thresh)) if mutant == 'thresh_ge' else (best > f32(c.thresh))
        w, h = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
        cx, cy = an[:, 0] + half * w, an[:, 1] + half * h
        dx, dy = r[:, 0] * std[0] + mean[0], r[:, 1] * std[1] + mean[1]
        dw, dh = r[:, 2] * std[2] + mean[2], r[:, 3] * std[3] + mean[3]
        wdx, hdy = w * dx, h * dy
        pcx, pcy = cx + wdx, cy + hdy
        pw, ph = w * np.exp(dw), h * np.exp(dh)
        assert pw.dtype == dt and pcx.dtype == dt
        x0, y0, x1, y1 = pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph
        x0, y0, x1, y1 = np.maximum(x0, xlo), np.maximum(y0, ylo), np.minimum(x1, xhi), np.minimum(y1, yhi)
        ex, ey = x1 - x0, y1 - y0
        keep = hit & (ex > 0) & (ey > 0)
        bx = U * (A_AFF * (np.abs(cx) + np.abs(wdx)) + B_EXP * pw)
        by = U * (A_AFF * (np.abs(cy) + np.abs(hdy)) + B_EXP * ph)
        idx = np.nonzero(keep)[0]
        out.append(dict(order=idx.astype(np.int32), classes=bk[idx].astype(np.int32), scores=best[idx],
                        boxes=np.stack([x0, y0, x1, y1], 1)[idx], bound=np.stack([bx, by, bx, by], 1)[idx].astype(f64),
                        extent=np.stack([ex, ey], 1)[hit].astype(f64), best=best, dwh=np.stack([dw, dh], 1)[hit].astype(f64)))
    return out


def decode_ref_of(c, d):
    return _decode(c, d, f64)


@functools.lru_cache(maxsize=None)
def _decode_ref(name):
    c = dcase(name)
    return decode_ref_of(c, decode_inputs(c))


def decode_ref(c):
    """computed once per case and shared: do not write to it"""
    return _decode_ref(c.name)


def decode_cand(c, ref):
    """the reference's candidates as the candidate lists nnl_nms reads (cap = A; boxes fp64 in randn mode, where the IoU condition is
    judged on them, and their exact fp32 values in grid mode)"""
    cand = dict(boxes=np.zeros((c.bs, c.A, 4)), classes=np.full((c.bs, c.A), -1, np.int32), scores=np.zeros((c.bs, c.A), f32),
                order=np.zeros((c.bs, c.A), np.int32), count=np.zeros(c.bs, np.int32))
    for i, r in enumerate(ref):
        n = len(r['order'])
        cand['boxes'][i, :n], cand['classes'][i, :n], cand['scores'][i, :n], cand['order'][i, :n] = r['boxes'], r['classes'], r['scores'], r['order']
        cand['count'][i] = n
    return cand


def decode_condition_failures(c, d):
    """the randn conditions a decode case must meet on its fp64 reference alone; a list of what fails"""
    bad = []
    ref = decode_ref_of(c, d)
    for i, r in enumerate(ref):
        if len(np.unique(r['scores'])) != len(r['scores']):
            bad.append('image %d: two candidates share a score' % i)
        b = r['best'][~np.isnan(r['best'])].astype(f64)
        if (np.abs(b - c.thresh) <= 1e-6 * c.thresh).any():
            bad.append('image %d: a best score within 1e-6 relative of thresh' % i)
        if (np.abs(r['extent']) < 1e-3).any():
            bad.append('image %d: a clipped extent within 1e-3 of 0' % i)
        if (np.abs(r['dwh']) > 1.5).any():
            bad.append('image %d: |dw| or |dh| above 1.5 (the bound assumes less)' % i)
    bad += nms_condition_failures(decode_cand(c, ref), c.top_k, c.max_overlap)
    return bad


# ---- NMS: inputs -----------------------------------------------------------------------------------------------------------------------------
def _disjoint(n):
    """n unit boxes on an integer grid, two apart: no two overlap"""
    i = np.arange(n)
    x, y = (i % 64) * 2.0, (i // 64) * 2.0
    return np.stack([x, y, x + 1, y + 1], 1).reshape(n, 4)


def _descending(n):
    """n distinct scores, exact in fp32, descending with the index"""
    return (1.0 - np.arange(n) / 4096.0).astype(f32)


CHAIN = ((0, 300, 10, 310), (2, 300, 12, 310), (4, 300, 14, 310))      # IoU(A,B) = IoU(B,C) = 2/3, IoU(A,C) = 3/7


def _image(spec, rs):
    """(boxes [n,4], classes [n], scores [n] f32, order [n]) of one image, in RANK order where the kind fixes one; make_cand shuffles the storage.
    rank       n disjoint boxes, scores k/64 with k in 1..max(2, n/12): groups of about 12 equal scores; order a permutation
    same       n identical boxes of one class; classes: n identical boxes of n classes
    pairs      n / 2 disjoint boxes, each twice with one class: the cut at top_k takes top_k / 2 pairs, of which one box each is kept
    chain      n - 3 disjoint fillers and CHAIN's A, B, C at the given ranks, class 0; fillers of classes 1, 2
    iou_eq     (0,0,4,4) and (0,0,4,2), same class: IoU exactly 1/2; n - 2 fillers
    zero_area  two identical zero-width boxes and two identical points, same class (0/0), n - 4 fillers
    signed_zero  n disjoint boxes, scores -0.0 at the even orders and +0.0 at the odd ones
    rand       n random boxes, 3 classes, distinct random scores"""
    kind, n = spec[0], spec[1]
    if kind == 'rank':
        levels = max(2, n // 12)
        return _disjoint(n)[rs.permutation(n)], rs.randint(0, 3, n), (rs.randint(1, levels + 1, n) / 64.0).astype(f32), rs.permutation(n)
    if kind == 'same':
        return np.tile([[3.0, 5.0, 9.0, 8.0]], (n, 1)), np.full(n, 2), _descending(n), rs.permutation(n)
    if kind == 'classes':
        return np.tile([[3.0, 5.0, 9.0, 8.0]], (n, 1)), rs.permutation(n), _descending(n), rs.permutation(n)
    if kind == 'pairs':
        return np.repeat(_disjoint(n // 2), 2, 0), np.repeat(rs.randint(0, 3, n // 2), 2), _descending(n), rs.permutation(n)
    if kind == 'chain':
        boxes, classes = _disjoint(n), rs.randint(1, 3, n)
        for p, b in zip(spec[2], CHAIN):
            boxes[p], classes[p] = b, 0
        return boxes, classes, _descending(n), rs.permutation(n)
    if kind == 'iou_eq':
        boxes, classes = _disjoint(n) + 100.0, np.zeros(n, int)
        boxes[1], boxes[3] = (0, 0, 4, 4), (0, 0, 4, 2)
        return boxes, classes, _descending(n), rs.permutation(n)
    if kind == 'zero_area':
        boxes, classes = _disjoint(n) + 100.0, np.zeros(n, int)
        boxes[0] = boxes[2] = (2, 2, 2, 3)
        boxes[1] = boxes[5] = (7, 7, 7, 7)
        return boxes, classes, _descending(n), rs.permutation(n)
    if kind == 'signed_zero':
        order = rs.permutation(n)
        return _disjoint(n), np.zeros(n, int), np.where(order % 2 == 0, f32(-0.0), f32(0.0)).astype(f32), order
    assert kind == 'rand'
    side = 4.0 * np.sqrt(max(n, 1))
    cx, cy, w, h = rs.uniform(0, side, n), rs.uniform(0, side, n), rs.uniform(4, 12, n), rs.uniform(4, 12, n)
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(f32).reshape(n, 4)
    return boxes, rs.randint(0, 3, n), rs.uniform(0.05, 1, n).astype(f32), rs.permutation(n)


def _build_cand(c, rs):
    imgs = [_image(s, rs) for s in c.images]
    cap = c.cap or max(1, max(s[1] for s in c.images))
    bs = len(imgs)
    cand = dict(boxes=np.zeros((bs, cap, 4), f32), classes=np.full((bs, cap), -1, np.int32), scores=np.zeros((bs, cap), f32),
                order=np.zeros((bs, cap), np.int32), count=np.zeros(bs, np.int32))
    for i, (b, k, s, o) in enumerate(imgs):
        n = len(s)
        st = rs.permutation(n)                                        # the storage order: any
        if c.null_order:                                              # the position is the order
            o = np.arange(n)
            st = np.arange(n) if c.images[i][0] != 'rand' else st
        cand['boxes'][i, :n], cand['classes'][i, :n], cand['scores'][i, :n], cand['order'][i, :n] = b[st], k[st], s[st], o[st]
        cand['count'][i] = n + 7 if 'over' in c.images[i][2:] else n   # a count above cap is read as cap (n == cap for that image)
        assert 'over' not in c.images[i][2:] or n == cap
    if c.null_order:
        cand['order'] = None
    return cand


@functools.lru_cache(maxsize=None)
def _nms_cand(name):
    c = ncase(name)
    for attempt in range(64):
        cand = _build_cand(c, np.random.RandomState(_seed(name) + attempt))
        if c.mode == 'grid' or not nms_condition_failures(cand, c.top_k, c.max_overlap):
            cand['attempt'] = attempt
            return _frozen(cand)
    raise AssertionError('%s: no seed meets the conditions' % name)


def nms_cand(c):
    """{boxes [bs,cap,4] f32, classes [bs,cap] i32, scores [bs,cap] f32, order [bs,cap] i32 or None, count [bs] i32} (shared: do not write)"""
    return _nms_cand(c.name)


def shuffled(cand, seed=5):
    """the same candidate multisets in another storage order (order must be given: it travels with its candidate)"""
    assert cand['order'] is not None
    out = {k: np.array(v) for k, v in cand.items() if isinstance(v, np.ndarray)}
    rs = np.random.RandomState(seed)
    for i in range(len(cand['count'])):
        n = min(int(cand['count'][i]), cand['scores'].shape[1])
        p = rs.permutation(n)
        for k in ('boxes', 'classes', 'scores', 'order'):
            out[k][i, :n] = cand[k][i, :n][p]
    return out


# ---- NMS: one arithmetic for the reference (fp64), the restatement (fp32) and the mutants -------------------------------------------------------
def _iou(b, dt):
    """[m,m] IoU in the kernel's operation order, every operation in dt"""
    b = b.astype(dt)
    iw = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), dt(0))
    ih = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), dt(0))
    inter = iw * ih
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = inter / ((area[:, None] + area[None, :]) - inter)
    assert iou.dtype == dt
    return iou


def _ranked(scores, order, n, top_k, mutant=None):
    """storage indices of the first top_k candidates under (score descending, order ascending); -0.0 == +0.0 as floats compare"""
    pos = np.arange(n)
    o = pos if order is None or mutant == 'tie_by_position' else order[:n]
    idx = np.lexsort((o, -scores[:n].astype(f64)))                   # the last key is the primary one; -(-0.0) == -(0.0)
    return idx if mutant == 'cut_after' else idx[:top_k]


def _nms_image(boxes, classes, scores, order, n, top_k, thr, dt, mutant=None):
    """storage indices of the kept candidates of one image, in rank order"""
    idx = _ranked(scores, order, n, top_k, mutant)
    m = len(idx)
    iou = _iou(boxes[idx], dt)
    with np.errstate(invalid='ignore'):
        over = (iou >= dt(thr)) if mutant == 'iou_ge' else (iou > dt(thr))
    if mutant != 'cross_class':
        over &= classes[idx][:, None] == classes[idx][None, :]
    kept, is_kept = [], np.zeros(m, bool)
    for j in range(m):
        by = np.ones(j, bool) if mutant == 'zombie' else is_kept[:j].copy()     # zombie: a suppressed box still suppresses
        if mutant == 'no_carry':
            by &= (np.arange(j) // KCHUNK) == j // KCHUNK                       # removals stay inside their 64-box chunk
        if not (over[:j, j] & by).any():
            kept.append(j)
            is_kept[j] = True
    kept = idx[np.array(kept, int)]
    return kept[:top_k] if mutant == 'cut_after' else kept


def nms_of(cand, top_k, thr, dt=f64, mutant=None):
    """the kept candidates as the C ABI returns them: {boxes [bs,top_k,4] f32, classes, scores, count}, SENTINEL past count.  The kept
    values are copies of the candidates' fp32 values (fp64 boxes of a decode reference are rounded: the caller compares those with the bound)"""
    bs, cap = cand['scores'].shape
    out = dict(boxes=np.full((bs, top_k, 4), SENTINEL, f32), classes=np.full((bs, top_k), INT_SENTINEL, np.int32),
               scores=np.full((bs, top_k), SENTINEL, f32), count=np.zeros(bs, np.int32), index=[])
    for i in range(bs):
        n = min(int(cand['count'][i]), cap)
        order = None if cand['order'] is None else cand['order'][i]
        k = _nms_image(cand['boxes'][i], cand['classes'][i], cand['scores'][i], order, n, top_k, thr, dt, mutant)
        out['boxes'][i, :len(k)], out['classes'][i, :len(k)], out['scores'][i, :len(k)] = cand['boxes'][i][k], cand['classes'][i][k], cand['scores'][i][k]
        out['count'][i] = len(k)
        out['index'].append(k)
    return out


def nms_ref_of(cand, top_k, thr):
    return nms_of(cand, top_k, thr, f64)


@functools.lru_cache(maxsize=None)
def _nms_ref(name):
    c = ncase(name)
    return nms_ref_of(nms_cand(c), c.top_k, c.max_overlap)


def nms_ref(c):
    """computed once per case and shared: do not write to it"""
    return _nms_ref(c.name)


def nms_condition_failures(cand, top_k, thr):
    """the randn conditions of an NMS input on its fp64 values alone: distinct scores per image, and no same-class pair of the ranked top_k
    with an IoU within 1e-4 of the threshold"""
    bad = []
    bs, cap = cand['scores'].shape
    for i in range(bs):
        n = min(int(cand['count'][i]), cap)
        s = cand['scores'][i, :n]
        if len(np.unique(s)) != n:
            bad.append('image %d: two candidates share a score' % i)
        idx = _ranked(s, None if cand['order'] is None else cand['order'][i], n, top_k)
        iou = _iou(cand['boxes'][i][idx], f64)
        same = cand['classes'][i][idx][:, None] == cand['classes'][i][idx][None, :]
        with np.errstate(invalid='ignore'):
            if (same & ~np.eye(len(idx), dtype=bool) & (np.abs(iou - float(f32(thr))) < 1e-4)).any():
                bad.append('image %d: a same-class IoU within 1e-4 of max_overlap' % i)
    return bad


def assert_conditions(c):
    """what the GPU test re-asserts before it judges a kernel by a randn case"""
    if c.mode != 'randn':
        return
    bad = decode_condition_failures(c, decode_inputs(c)) if isinstance(c, DCase) else nms_condition_failures(nms_cand(c), c.top_k, c.max_overlap)
    assert not bad, '%s does not meet its conditions: %s' % (c.name, bad)


# ---- the merge into NMS ------------------------------------------------------------------------------------------------------------------------
UNDO = np.dtype([('col_jit', '<f4'), ('row_jit', '<f4'), ('inv', '<f4'), ('cols', '<f4'), ('flip', '<i4')])
MERGE_TOP_K, MERGE_OVERLAP = 100, 0.5


@functools.lru_cache(maxsize=None)
def merge_inputs(P):
    """L = 3 images (image 1: every count 0), P passes, M slots: integer boxes, jitters 0..8, inv in (1/2, 1, 2), scores k/16 (ties across the passes)"""
    L, M = 3, 70 if P == 1 else 5
    rs = np.random.RandomState(900 + P)
    x0, y0 = rs.randint(8, 40, (L, P, M)), rs.randint(8, 40, (L, P, M))
    boxes = np.stack([x0, y0, x0 + rs.randint(2, 12, (L, P, M)), y0 + rs.randint(2, 12, (L, P, M))], 3).astype(f32)
    classes = rs.randint(0, 2, (L, P, M)).astype(np.int32)
    scores = np.sort(rs.randint(1, 16, (L, P, M)) / 16.0, axis=2)[:, :, ::-1].astype(f32)       # descending inside a pass
    counts = rs.randint(0, M + 1, (L, P)).astype(np.int32)
    counts[1] = 0
    counts[2, ::3] = 0
    counts[0, 0] = M
    undo = np.zeros((L, P), UNDO)
    undo['col_jit'], undo['row_jit'] = rs.randint(0, 9, (L, P)), rs.randint(0, 9, (L, P))
    undo['inv'], undo['cols'], undo['flip'] = np.array((0.5, 1.0, 2.0), f32)[rs.randint(0, 3, (L, P))], 64.0, rs.randint(0, 2, (L, P))
    return _frozen(dict(boxes=np.ascontiguousarray(boxes), classes=classes, scores=np.ascontiguousarray(scores), counts=counts, undo=undo, L=L, P=P, M=M))


def merge_ref(m):
    """the candidate lists nnl_tta_bbox_merge writes, fillers included (box 0, class -1, score 0, order = position)"""
    L, P, M = m['L'], m['P'], m['M']
    cap = P * M
    cand = dict(boxes=np.zeros((L, cap, 4), f32), classes=np.full((L, cap), -1, np.int32), scores=np.zeros((L, cap), f32),
                order=np.tile(np.arange(cap, dtype=np.int32), (L, 1)), count=np.zeros(L, np.int32))
    for l in range(L):
        d = 0
        for p in range(P):
            u = m['undo'][l, p]
            for r in range(int(m['counts'][l, p])):
                b = m['boxes'][l, p, r]
                x0, y0, x1, y1 = (b[0] - u['col_jit']) * u['inv'], (b[1] - u['row_jit']) * u['inv'], (b[2] - u['col_jit']) * u['inv'], (b[3] - u['row_jit']) * u['inv']
                if u['flip']:
                    x0, x1 = u['cols'] - x1, u['cols'] - x0
                cand['boxes'][l, d], cand['classes'][l, d], cand['scores'][l, d] = (x0, y0, x1, y1), m['classes'][l, p, r], m['scores'][l, p, r]
                d += 1
        cand['count'][l] = d
    return cand


# ---- the same arithmetic in numpy fp32: validates the checks, judges nothing ------------------------------------------------------------------------
def restate32_decode(c):
    """the candidates as a correct fp32 evaluation gives them, in the layout of the C ABI's outputs (storage in REVERSED anchor order: the
    append order is not defined, check_decode must not depend on it)"""
    return decode_as_returned(c, _decode(c, decode_inputs(c), f32), reverse=True)


def decode_as_returned(c, per_image, reverse=False):
    got = dict(boxes=np.full((c.bs, c.A, 4), SENTINEL, f32), classes=np.full((c.bs, c.A), INT_SENTINEL, np.int32),
               scores=np.full((c.bs, c.A), SENTINEL, f32), order=np.full((c.bs, c.A), INT_SENTINEL, np.int32), count=np.zeros(c.bs, np.int32))
    for i, r in enumerate(per_image):
        n = len(r['order'])
        s = slice(None, None, -1) if reverse else slice(None)
        got['boxes'][i, :n], got['classes'][i, :n], got['scores'][i, :n], got['order'][i, :n] = r['boxes'][s].astype(f32), r['classes'][s], r['scores'][s], r['order'][s]
        got['count'][i] = n
    return got


def restate32_nms(cand, top_k, thr):
    return nms_of(cand, top_k, thr, f32)


def restate32(c):
    """a case of either table as a correct fp32 evaluation returns it"""
    return restate32_decode(c) if isinstance(c, DCase) else restate32_nms(nms_cand(c), c.top_k, c.max_overlap)


NMS_MUTANTS = ('zombie', 'cross_class', 'iou_ge', 'tie_by_position', 'cut_after', 'no_carry')
DECODE_MUTANTS = ('last_max', 'thresh_ge', 'window_lo_ignored')


# ---- the checks (what the GPU test applies to the kernels, and the CPU test to restate32 and the mutants) -----------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _untouched(name, a, count, fill, what):
    for i in range(len(count)):
        rest = a[i, int(count[i]):]
        assert (_bits(rest) == _bits(np.array(fill, a.dtype))).all(), '%s: image %d: %s was written at or beyond its count %d' % (name, i, what, count[i])


def check_decode(c, ref, got):
    """count exactly; after sorting by cand_order: the anchors, classes and scores exactly, the boxes bit for bit (grid) or within the bound
    (randn); every slot at or beyond the count still holds its sentinel.  Returns the worst err / bound (0 in grid mode)."""
    worst = 0.0
    want_n = np.array([len(r['order']) for r in ref], np.int32)
    assert got['count'].dtype == np.int32 and np.array_equal(got['count'], want_n), '%s: cand_count %s, reference %s' % (c.name, got['count'], want_n)
    for k, fill in (('boxes', SENTINEL), ('scores', SENTINEL), ('classes', INT_SENTINEL), ('order', INT_SENTINEL)):
        _untouched(c.name, got[k], want_n, fill, 'cand_' + k)
    for i, r in enumerate(ref):
        n = int(want_n[i])
        p = np.argsort(got['order'][i, :n], kind='stable')
        ctx = '%s: image %d' % (c.name, i)
        assert np.array_equal(got['order'][i, :n][p], r['order']), '%s: the candidates are not the reference\'s anchors' % ctx
        bad = np.nonzero(got['classes'][i, :n][p] != r['classes'])[0]
        assert len(bad) == 0, '%s: anchor %d: class %d, reference %d' % (ctx, r['order'][bad[0]], got['classes'][i, :n][p][bad[0]], r['classes'][bad[0]])
        assert np.array_equal(_bits(got['scores'][i, :n][p]), _bits(r['scores'])), '%s: a score is not the bitwise copy of the best class score' % ctx
        b = got['boxes'][i, :n][p]
        if c.mode == 'grid':
            assert np.array_equal(r['boxes'].astype(f32).astype(f64), r['boxes']), '%s: the grid reference is not exact in fp32' % ctx
            bad = np.argwhere(_bits(b) != _bits(r['boxes'].astype(f32)))
            assert len(bad) == 0, '%s: anchor %d: box %s, reference %s' % (ctx, r['order'][bad[0][0]] if len(bad) else -1, b[bad[0][0]] if len(bad) else None,
                                                                          r['boxes'][bad[0][0]] if len(bad) else None)
        elif n:
            assert np.isfinite(b).all(), '%s: a box is not finite' % ctx
            q = np.abs(b.astype(f64) - r['boxes']) / r['bound']
            j = np.unravel_index(np.argmax(q), q.shape)
            assert q[j] <= 1, '%s: anchor %d coordinate %d: %r, fp64 %r: err / bound %.3f' % (ctx, r['order'][j[0]], j[1], b[j], r['boxes'][j], q[j])
            worst = max(worst, float(q[j]))
    return worst


def check_nms(name, ref, got, boxes_exact=True):
    """kept_count, and the kept boxes, classes and scores bit for bit (copies of the candidates); every slot at or beyond kept_count still
    holds its sentinel.  boxes_exact=False (decode into NMS, randn): the caller compares the boxes with the decode bound."""
    assert got['count'].dtype == np.int32 and np.array_equal(got['count'], ref['count']), '%s: kept_count %s, reference %s' % (name, got['count'], ref['count'])
    for k, fill in (('boxes', SENTINEL), ('scores', SENTINEL), ('classes', INT_SENTINEL)):
        _untouched(name, got[k], ref['count'], fill, 'kept_' + k)
    for i, n in enumerate(ref['count']):
        for k in ('classes', 'scores') + (('boxes',) if boxes_exact else ()):
            bad = np.argwhere(_bits(got[k][i, :n]) != _bits(ref[k][i, :n]))
            assert len(bad) == 0, '%s: image %d: kept_%s differs from rank %d on: %s, reference %s' % (
                name, i, k, bad[0][0] if len(bad) else -1, got[k][i, :n][bad[0][0]] if len(bad) else None, ref[k][i, :n][bad[0][0]] if len(bad) else None)


def check_kept_boxes_within_bound(c, dref, nref, got):
    """decode into NMS, randn: kept box j of image i is the decode of anchor dref[i].order[nref.index[i][j]]: within that anchor's bound"""
    worst = 0.0
    for i in range(c.bs):
        k = nref['index'][i]
        if len(k):
            q = np.abs(got['boxes'][i, :len(k)].astype(f64) - dref[i]['boxes'][k]) / dref[i]['bound'][k]
            assert q.max() <= 1, '%s: image %d: a kept box is off its anchor\'s decode: err / bound %.3f' % (c.name, i, q.max())
            worst = max(worst, float(q.max()))
    return worst


def same_bits(a, b, ctx):
    for k in ('boxes', 'classes', 'scores', 'count'):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), '%s: %s differs' % (ctx, k)


# ---- regimes: named predicates; a decode regime sees (case, inputs, reference), an NMS regime (case, candidates, reference) ------------------------------
def _best_rows(c, d):
    """(image, anchor) rows of clas with their first maximum, NaN rows excluded"""
    for i in range(c.bs):
        clas = d['clas'][i]
        ok = ~np.isnan(clas).any(1)
        yield i, clas, ok, clas.max(1)


def _tie(c, d, r, k):
    """an anchor above thresh whose maximum is shared by exactly k classes, and that is a candidate"""
    for i, clas, ok, best in _best_rows(c, d):
        with np.errstate(invalid='ignore'):
            hit = ok & (best > f32(c.thresh)) & ((clas == best[:, None]).sum(1) == k)
        if np.isin(np.nonzero(hit)[0], r[i]['order']).any():
            return True
    return False


def _score_at(c, d, r, v, kept):
    for i, clas, ok, best in _best_rows(c, d):
        a = np.nonzero(ok & (best == v))[0]
        if len(a) and (np.isin(a, r[i]['order']).any() if kept else not np.isin(a, r[i]['order']).any()):
            return True
    return False


def _nan_would_pass(c, d, r):
    """an anchor with a NaN score whose other scores alone would make it a candidate, NaN in the first / a later class"""
    first = later = False
    for i in range(c.bs):
        clas = d['clas'][i]
        nan = np.isnan(clas)
        with np.errstate(invalid='ignore'):
            rows = nan.any(1) & (np.where(nan, -np.inf, clas).max(1) > c.thresh) if c.K > 1 else nan.any(1)
        first |= bool((rows & nan[:, 0]).any())
        later |= bool((rows & ~nan[:, 0]).any())
        assert not np.isin(np.nonzero(nan.any(1))[0], r[i]['order']).any()
    return first and later


def _edge_dropped(j):
    def pred(c, d, r):
        if not (c.mode == 'grid' and c.edges):
            return False
        a = c.A - len(EDGE_ANCHORS) + j
        return any(kind_of(c, i) == 'mixed' and d['clas'][i, a].max() > c.thresh and a not in r[i]['order'] for i in range(c.bs))
    return pred


def _window_inner(c, d, r):
    x0, y0, x1, y1 = window_of(c)
    if not (x0 > 0 and y0 > 0 and x1 < IMG and y1 < IMG):
        return False
    b = np.concatenate([q['boxes'] for q in r])
    on = [(b[:, 0] == x0).any(), (b[:, 1] == y0).any(), (b[:, 2] == x1).any(), (b[:, 3] == y1).any()]
    whole = _decode(c._replace(window=None), d, f64)                  # anchors the image keeps and this window drops
    return all(on) and sum(len(q['order']) for q in whole) > sum(len(q['order']) for q in r)


def _n_of(cand, i):
    return min(int(cand['count'][i]), cand['scores'].shape[1])


def _m_of(c, cand, i):
    return min(_n_of(cand, i), c.top_k)


def _any_image(f):
    return lambda c, cand, r: any(f(c, cand, r, i) for i in range(len(cand['count'])))


def _rank_n(n):
    return _any_image(lambda c, cand, r, i: c.images[i][0] == 'rank' and _n_of(cand, i) == n)


def _cut_in_group(c, cand, r, i):
    """the cut at top_k falls inside a group of equal scores, and taking the group's members by position would take others"""
    n = _n_of(cand, i)
    if n <= c.top_k:
        return False
    order = None if cand['order'] is None else cand['order'][i]
    full = _ranked(cand['scores'][i], order, n, n)
    s = cand['scores'][i][full]
    return s[c.top_k - 1] == s[c.top_k] and (order is None or set(_ranked(cand['scores'][i], None, n, c.top_k)) != set(full[:c.top_k]))


def _m_is(m):
    return _any_image(lambda c, cand, r, i: _m_of(c, cand, i) == m)


def _suppression_across_chunks(c, cand, r, i):
    """a box removed by a kept box of an EARLIER 64-box chunk and by no kept box of its own"""
    return c.mode == 'randn' and r['count'][i] != nms_of({k: (v[i:i + 1] if isinstance(v, np.ndarray) else v) for k, v in cand.items()},
                                                       c.top_k, c.max_overlap, f64, 'no_carry')['count'][0]


def _kind(k, extra=lambda c, cand, r, i: True):
    return _any_image(lambda c, cand, r, i: c.images[i][0] == k and extra(c, cand, r, i))


def _chain_ranks(across):
    def f(c, cand, r, i):
        a, b, cc = (p // KCHUNK for p in c.images[i][2])
        kept = {tuple(x) for x in r['boxes'][i, :r['count'][i]][r['classes'][i, :r['count'][i]] == 0]}
        ok = kept == {tuple(f32(v) for v in CHAIN[0]), tuple(f32(v) for v in CHAIN[2])}           # A and C kept, B suppressed
        return ok and ((a == 0 and b >= 1 and cc >= 1) if across else (a == b == cc))
    return f


DECODE_REGIMES = collections.OrderedDict([
    ('decode A < 256', lambda c, d, r: c.A < KDECODE),
    ('decode A % 256 == 0', lambda c, d, r: c.A % KDECODE == 0),
    ('decode A % 256 != 0, A > 256', lambda c, d, r: c.A % KDECODE != 0 and c.A > KDECODE),
    ('decode A % 256 == 1 (a block of one anchor)', lambda c, d, r: c.A % KDECODE == 1),
    ('decode about 2100 anchors', lambda c, d, r: c.A >= 2048),
    ('decode K == 1', lambda c, d, r: c.K == 1),
    ('decode grid: two classes share the maximum', lambda c, d, r: c.mode == 'grid' and _tie(c, d, r, 2)),
    ('decode grid: three classes share the maximum', lambda c, d, r: c.mode == 'grid' and _tie(c, d, r, 3)),
    ('decode grid: a score equal to thresh is dropped', lambda c, d, r: c.mode == 'grid' and _score_at(c, d, r, GRID_THRESH, False)),
    ('decode grid: the next fp32 above thresh is kept', lambda c, d, r: c.mode == 'grid' and _score_at(c, d, r, ABOVE_THRESH, True)),
    ('decode NaN score in the first and in a later class', _nan_would_pass),
    ('decode batch >= 3 with an image of zero candidates', lambda c, d, r: c.bs >= 3 and any(len(q['order']) == 0 for q in r)),
    ('decode batch >= 3 with count == A', lambda c, d, r: c.bs >= 3 and any(len(q['order']) == c.A for q in r)),
    ('decode box wholly outside', _edge_dropped(0)),
    ('decode zero width at the lower bound', _edge_dropped(1)),
    ('decode zero width at the upper bound', _edge_dropped(2)),
    ('decode zero height at the lower bound', _edge_dropped(3)),
    ('decode window strictly inside, boxes on all four edges', _window_inner),
    ('decode window equal to the image', lambda c, d, r: c.window == (0.0, 0.0, IMG, IMG)),
    ('decode randn', lambda c, d, r: c.mode == 'randn'),
    ('decode randn with a window', lambda c, d, r: c.mode == 'randn' and c.window is not None),
])
NMS_REGIMES = collections.OrderedDict(
    [('rank n == %d' % n, _rank_n(n)) for n in (0, 1, 255, 256, 257, 1023, 1024, 1025, 2100)] + [
        ('rank top_k below n', _any_image(lambda c, cand, r, i: c.top_k < _n_of(cand, i))),
        ('rank top_k equal to n', _any_image(lambda c, cand, r, i: c.top_k == _n_of(cand, i))),
        ('rank top_k above n', _any_image(lambda c, cand, r, i: c.top_k > _n_of(cand, i) > 0)),
        ('rank top_k above cap', lambda c, cand, r: c.top_k > cand['scores'].shape[1]),
        ('rank the cut inside a group of equal scores, order permuted', lambda c, cand, r: cand['order'] is not None and _any_image(_cut_in_group)(c, cand, r)),
        ('rank the cut inside a group of equal scores, order NULL', lambda c, cand, r: cand['order'] is None and _any_image(_cut_in_group)(c, cand, r)),
        ('rank order NULL beyond one LDS tile', lambda c, cand, r: cand['order'] is None and cand['scores'].shape[1] > KRANKTILE),
        ('rank batch: counts 0, cap and above cap', lambda c, cand, r: len(cand['count']) >= 3 and 0 in cand['count'] and any(
            cand['count'] == cand['scores'].shape[1]) and any(cand['count'] > cand['scores'].shape[1])),
        ('rank -0.0 and +0.0 are one score', _kind('signed_zero')),
    ] + [('scan survivors m == %d' % m, _m_is(m)) for m in (1, 63, 64, 65, 128, 129)] + [
        ('scan survivors m >= 193', _any_image(lambda c, cand, r, i: _m_of(c, cand, i) >= 193)),
        ('scan top_k == 64', lambda c, cand, r: c.top_k == 64),
        ('scan top_k % 64 != 0 and m == top_k', _any_image(lambda c, cand, r, i: c.top_k % 64 != 0 and _m_of(c, cand, i) == c.top_k)),
        ('scan top_k == 200', lambda c, cand, r: c.top_k == 200),
        ('scan all disjoint: kept_count == m', _any_image(lambda c, cand, r, i: c.images[i][0] == 'rank' and r['count'][i] == _m_of(c, cand, i) >= 193)),
        ('scan all identical, one class: one kept', _kind('same', lambda c, cand, r, i: r['count'][i] == 1 and _m_of(c, cand, i) >= 193)),
        ('scan the cut comes before the suppression', _kind('pairs', lambda c, cand, r, i: _n_of(cand, i) >= 2 * c.top_k and r['count'][i] == c.top_k // 2)),
        ('scan identical boxes of different classes: all kept', _kind('classes', lambda c, cand, r, i: r['count'][i] == _m_of(c, cand, i) == 65)),
        ('scan chain across a chunk boundary, C in chunk 1', _kind('chain', lambda c, cand, r, i: _chain_ranks(True)(c, cand, r, i) and c.images[i][2][2] // 64 == 1)),
        ('scan chain across a chunk boundary, C in chunk 2', _kind('chain', lambda c, cand, r, i: _chain_ranks(True)(c, cand, r, i) and c.images[i][2][2] // 64 == 2)),
        ('scan chain inside one chunk', _kind('chain', _chain_ranks(False))),
        ('scan IoU equal to max_overlap: kept', _kind('iou_eq', lambda c, cand, r, i: c.max_overlap == 0.5 and r['count'][i] == _n_of(cand, i))),
        ('scan IoU one ulp above max_overlap: suppressed', _kind('iou_eq', lambda c, cand, r, i: c.max_overlap == float(BELOW_HALF) and r['count'][i] == _n_of(cand, i) - 1)),
        ('scan zero-area pair: 0/0 suppresses nothing', _kind('zero_area', lambda c, cand, r, i: r['count'][i] == _n_of(cand, i))),
        ('scan randn: suppression carried across chunks', _any_image(_suppression_across_chunks)),
        ('scan randn with order NULL', lambda c, cand, r: c.mode == 'randn' and cand['order'] is None),
        ('scan batch with an empty image between others', lambda c, cand, r: c.mode == 'randn' and 0 in list(cand['count'][1:-1])),
    ])
REGIMES = collections.OrderedDict(list(DECODE_REGIMES.items()) + list(NMS_REGIMES.items()))


def coverage():
    """{regime: [names of the cases that reach it]}"""
    cov = collections.OrderedDict((k, []) for k in REGIMES)
    for c in DECODE_CASES:
        d, r = decode_inputs(c), decode_ref(c)
        for k, pred in DECODE_REGIMES.items():
            if pred(c, d, r):
                cov[k].append(c.name)
    for c in NMS_CASES:
        cand, r = nms_cand(c), nms_ref(c)
        for k, pred in NMS_REGIMES.items():
            if pred(c, cand, r):
                cov[k].append(c.name)
    return cov
