"""The geometry list of the conv C-ABI sweep (tests/test_conv_abi_gpu.py, tests/test_conv_cases_cpu.py) and its reference.

A plain module: no fixtures, nothing from the library.  `python -m tests.conv_cases` prints the list.

A case is (N, C, H, W, K, R, S, stride, pad) in nn.Conv2d's terms (one stride, one symmetric padding), plus a name, what it is for, and —
for the few cases that reach a route through an existing switch — the NNL_* environment it runs under.  HAND is written out, GENERATED
fills the product filter x stride x padding class with sizes / channels / batch drawn by a seeded generator; CASES is both, hand-written
first (ordered by theme; the sweep runs each part small to large).

The reference is torch.nn.functional.conv2d and its autograd in fp64 on the CPU.

Data modes:
  int    small integers (weights never zero).  Every product and partial sum of every kernel is then exactly representable in fp32 — the
         Winograd transforms included (constants +-1, +-1/2: all intermediates are multiples of 1/4) — so a correct kernel reproduces the
         fp64 reference BIT FOR BIT in any summation order and at any split-K.  int_ranges() derives the magnitude bound per case.
  randn  the project's scaling (w / sqrt(C*R*S)) and tolerance (rtol 1e-4, atol 1e-5 * max|ref| per tensor): notices a precision downgrade,
         which small integers cannot (they are exact in bf16 / xf32 too).
"""
import collections
import random

import torch
import torch.nn.functional as F

Case = collections.namedtuple('Case', 'N C H W K R S stride pad name why env')

RTOL, ATOL_REL = 1e-4, 1e-5                     # the project's tolerance for these kernels (test_conv2d_fwd_bwd, every Winograd test)
FLOP_CAP, FLOP_CAP_NAMED, FLOP_CAP_LIST = 2e9, 2e10, 1e11
MAX_ELEMS = 1 << 28
IGEMM_MAX_TAPS = 49

FILTERS = [(1, 1), (3, 3), (5, 5), (7, 7), (2, 2), (4, 4), (1, 3), (3, 1), (1, 7), (7, 1), (9, 9), (1, 33), (1, 49)]
STRIDES = [1, 2, 3]
SIZES = [1, 2, 3, 5, 7, 8, 13, 16, 17, 28, 31, 33, 56]
CHANNELS = [4, 8, 12, 16, 20, 36, 44, 48, 64, 80, 100, 128, 180, 256, 512]
BATCHES = [1, 2, 3, 5, 17]


def out_size(H, R, stride, pad):
    """nn.Conv2d's output size (floor division); <= 0 or a filter larger than the padded input is not a legal geometry"""
    return (H + 2 * pad - R) // stride + 1 if H + 2 * pad >= R else 0


def PQ(c):
    return out_size(c.H, c.R, c.stride, c.pad), out_size(c.W, c.S, c.stride, c.pad)


def valid(c):
    """what csrc/conv2d.hip's check_geom accepts"""
    P, Q = PQ(c)
    return (min(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.stride) > 0 and c.pad >= 0 and P > 0 and Q > 0 and c.C % 4 == 0 and
            c.N * c.H * c.W * c.C < 1 << 31 and c.N * P * Q * c.K < 1 << 31 and c.N * P * Q < 1 << 30)


def flop(c):
    P, Q = PQ(c)
    return 2.0 * c.N * P * Q * c.K * c.R * c.S * c.C


def case_id(c):
    return '%s-n%dc%d-%dx%d-k%d-%dx%d-s%dp%d' % (c.name, c.N, c.C, c.H, c.W, c.K, c.R, c.S, c.stride, c.pad)


def _c(name, N, C, H, W, K, R, S, stride, pad, why, env=None):
    return Case(N, C, H, W, K, R, S, stride, pad, name, why, dict(env or {}))


# ---- the hand-written part: what each case is for ---------------------------------------------------------------------------------
HAND = [
    # padding classes the suite never ran
    _c('pad0-3x3', 2, 16, 8, 7, 16, 3, 3, 1, 0, 'a 3x3 without padding: no border tap at all'),
    _c('pad2-3x3', 2, 16, 8, 7, 16, 3, 3, 1, 2, 'pad = R - 1: every border output sees two padded rows'),
    _c('pad1-1x1', 2, 32, 7, 5, 32, 1, 1, 1, 1, 'a 1x1 with pad 1: the border ring of the output is the bias'),
    _c('pad1-1x1-s2', 3, 32, 7, 8, 48, 1, 1, 2, 1, 'a 1x1 / stride 2 with pad 1: the dgrad has parity classes without a tap (need_zero)'),
    _c('pad-ge-R', 2, 16, 5, 5, 16, 3, 3, 1, 4, 'pad >= R: outputs that see only padding must equal the bias'),
    _c('pad-ge-R-s2', 2, 16, 5, 4, 32, 3, 3, 2, 3, 'pad >= R at stride 2'),
    _c('pad130', 1, 16, 4, 4, 16, 3, 3, 1, 130, 'tap offset dh = 130 at stride 1: past signed char, the affine integers carry it'),
    _c('pad260-s2', 1, 16, 4, 4, 16, 3, 3, 2, 260, 'tap offset dh = 130 at stride 2: past the signed char of the dgrad tap table'),
    _c('H-lt-R', 2, 16, 1, 2, 16, 5, 5, 1, 2, 'H < R made legal by padding; P == 1'),
    _c('Q-eq-1', 2, 20, 9, 3, 12, 3, 3, 1, 0, 'Q == 1, C and K multiples of 4 only: the row-k kernel'),
    # rectangular and large filters
    _c('1x33', 1, 16, 3, 56, 16, 1, 33, 1, 0, 'a 1 x 33 raster: the affine tap mask shifts a 32-bit one by 32'),
    _c('1x33-pad', 2, 16, 2, 33, 32, 1, 33, 1, 16, '1 x 33 with same padding, dgrad through the tap table'),
    _c('1x49', 1, 16, 2, 56, 16, 1, 49, 1, 24, 'a 1 x 49 raster: IGEMM_MAX_TAPS taps in one row'),
    _c('1x49-s2', 1, 32, 3, 56, 16, 1, 49, 2, 24, '1 x 49 at stride 2: parity classes of 24 / 25 taps'),
    _c('49x1', 1, 16, 56, 2, 16, 49, 1, 1, 24, 'the transposed raster: 49 rows of one column'),
    _c('9x9', 1, 16, 13, 13, 16, 9, 9, 1, 4, '81 taps: over IGEMM_MAX_TAPS, the row-k kernel although C % 16 == 0'),
    _c('9x9-s2', 2, 8, 17, 13, 12, 9, 9, 2, 4, '81 taps at stride 2'),
    _c('7x7-s3', 2, 16, 31, 28, 32, 7, 7, 3, 3, 'stride 3: the dgrad has no tap-table launch for it'),
    _c('4x4-s2', 2, 32, 16, 16, 32, 4, 4, 2, 1, 'even filter at stride 2: four parity classes of four taps, merged'),
    _c('4x4-s2-odd', 2, 32, 17, 13, 32, 4, 4, 2, 1, 'the same on odd sizes: one launch per class; (H + 2 pad - R) % stride != 0'),
    _c('2x2-s2', 3, 16, 8, 8, 16, 2, 2, 2, 0, '2x2 / stride 2: one tap per parity class'),
    _c('3x3-s2-tail', 2, 32, 8, 8, 32, 3, 3, 2, 0, 'trailing input row / column receives no gradient'),
    _c('3x3-s3-tail', 2, 16, 8, 7, 16, 3, 3, 3, 0, 'stride 3 with trailing rows that receive no gradient'),
    _c('1x1-s3', 2, 64, 8, 7, 64, 1, 1, 3, 0, 'a 1x1 at stride 3: most dx pixels receive nothing'),
    # channel switches: tap table (C % 16), KTAIL (one tap, C % 4, >= 32), row-k (the rest)
    _c('ktail16', 2, 36, 8, 8, 64, 1, 1, 1, 0, 'one tap, C = 36: KTAIL with the 16-wide k block; dgrad (K = 64) on the tap table'),
    _c('ktail32', 2, 100, 8, 8, 44, 1, 1, 1, 0, 'one tap, C = 100: KTAIL with the 32-wide k block; dgrad KTAIL 16 (K = 44)'),
    _c('ktail-bal', 1, 500, 32, 32, 1000, 1, 1, 1, 0, '1024 x 500 x 1000: few long tiles, KTAIL under the balanced schedule'),
    _c('rowk-1x1-c20', 2, 20, 8, 8, 20, 1, 1, 1, 0, 'one tap, C = 20 < 32: neither tap table nor KTAIL'),
    _c('rowk-c4', 5, 4, 13, 13, 4, 3, 3, 1, 1, 'C = K = 4'),
    _c('rowk-c180', 2, 180, 7, 7, 36, 3, 3, 1, 1, 'C = 180, K = 36: row-k in both directions'),
    # tile shapes of the tap-table kernel (the cost formula of dispatch_taps) and of the row-k kernel (block counts)
    _c('taps128x128-onetap', 1, 16, 32, 32, 8192, 1, 1, 1, 0, 'one tap, Nc >= 8192, M >= 1024: the 128 x 128 rule'),
    _c('bal-off', 8, 128, 14, 14, 256, 3, 3, 1, 1, 'NNL_IGEMM_BALANCE=0: the plain grid on a shape the balanced schedule takes',
       {'NNL_IGEMM_BALANCE': '0', 'NNL_CONV_WINO': '0'}),
    _c('bal-force', 8, 256, 14, 14, 256, 3, 3, 2, 1, 'NNL_IGEMM_BALANCE=2 forces a sliced plan', {'NNL_IGEMM_BALANCE': '2', 'NNL_CONV_WINO': '0'}),
    # 3x3 / stride 1 / pad 1 where nnl_conv2d_wino_preferred answers 0, 1, 2; odd W and odd H
    _c('wino-none', 1, 16, 5, 3, 8, 3, 3, 1, 1, 'too small for either Winograd kernel: preferred == 0'),
    _c('wino1d-forced', 2, 64, 12, 10, 64, 3, 3, 1, 1, 'NNL_CONV_WINO=2: the 1-D kernel, even width', {'NNL_CONV_WINO': '2'}),
    _c('wino1d-forced-odd', 3, 32, 9, 7, 36, 3, 3, 1, 1, 'NNL_CONV_WINO=2: the 1-D kernel, odd width and height', {'NNL_CONV_WINO': '2'}),
    _c('wino1d-ksliced', 4, 128, 14, 14, 128, 3, 3, 1, 1, 'the 1-D kernel with forced k slices', {'NNL_CONV_WINO': '2', 'NNL_WINO_PLAN_KS': '2', 'NNL_WINO_PLAN_S': '4'}),
    _c('wino1d-bk16-ksliced', 4, 48, 14, 14, 48, 3, 3, 1, 1, 'the 1-D kernel with C = K = 48 (16-wide k block) and forced k slices, both directions',
       {'NNL_CONV_WINO': '2', 'NNL_WINO_PLAN_KS': '2', 'NNL_WINO_PLAN_S': '4'}),
    _c('wino2d-forced-odd', 2, 64, 17, 33, 96, 3, 3, 1, 1, 'NNL_CONV_WINO=3: the 2-D kernel on odd sizes', {'NNL_CONV_WINO': '3', 'NNL_WINO2_POS': '0'}),
    _c('wino2d-bk16', 2, 48, 13, 16, 48, 3, 3, 1, 1, 'the 2-D kernel with C % 32 != 0: the 16-wide k block', {'NNL_CONV_WINO': '3', 'NNL_WINO2_POS': '0'}),
    _c('wino2d-ksliced', 4, 128, 14, 14, 128, 3, 3, 1, 1, 'the 2-D kernel with forced k slices',
       {'NNL_CONV_WINO': '3', 'NNL_WINO2_POS': '0', 'NNL_WINO_PLAN_KS': '2', 'NNL_WINO_PLAN_S': '4'}),
    _c('wino2d-pos', 8, 256, 14, 14, 256, 3, 3, 1, 1, 'the position-split plan of the 2-D kernel', {'NNL_CONV_WINO': '3', 'NNL_WINO2_POS': '2'}),
    _c('wino-default-8x512x7', 8, 512, 7, 7, 512, 3, 3, 1, 1, 'ResNet-34 layer4 at 8 images under the default planner'),
    _c('wino-default-odd', 5, 64, 31, 33, 64, 3, 3, 1, 1, 'odd H and W, default planner'),
    _c('wgrad-wino-off', 5, 64, 31, 33, 64, 3, 3, 1, 1, 'NNL_WGRAD_WINO=0: the direct weight gradient on a Winograd-domain shape', {'NNL_WGRAD_WINO': '0'}),
    _c('wgrad-wino1d', 5, 64, 28, 28, 64, 3, 3, 1, 1, 'NNL_WGRAD_WINO=2, NNL_WGRAD_WINO2D=0: the 1-D Winograd-domain weight gradient',
       {'NNL_WGRAD_WINO': '2', 'NNL_WGRAD_WINO2D': '0'}),
    _c('wgrad-wino2d', 5, 64, 17, 33, 48, 3, 3, 1, 1, 'NNL_WGRAD_WINO2D=2: the 2-D Winograd-domain weight gradient on odd sizes', {'NNL_WGRAD_WINO2D': '2'}),
    # large M under the default planner: 128-row tiles, balanced schedule with main_ks > 1 / tail slices, wgrad split-K
    _c('bigM-1x1', 17, 64, 56, 56, 128, 1, 1, 1, 0, 'N*P*Q = 53 312, one tap'),
    _c('bigM-3x3-c16', 5, 16, 112, 112, 64, 3, 3, 1, 1, 'N*P*Q = 62 720, C = 16'),
    _c('bigM-3x3', 17, 32, 56, 56, 64, 3, 3, 1, 1, 'N*P*Q = 53 312, 3x3 / pad 1: the Winograd planners on a large grid'),
    _c('bigM-k256', 17, 64, 56, 56, 256, 1, 1, 1, 0, 'N*P*Q = 53 312, K = 256'),
    _c('bigM-ktail', 17, 100, 56, 56, 128, 1, 1, 1, 0, 'KTAIL on a grid of 1666 tiles'),
    _c('bigM-rowk', 17, 12, 58, 58, 128, 3, 3, 1, 0, 'N*P*Q = 53 312 on the row-k kernel: its 128 x 128 tile (>= 400 blocks)'),
    _c('rowk64x128', 17, 12, 42, 42, 128, 3, 3, 1, 0, 'N*P*Q = 27 200 on the row-k kernel: 425 blocks of 64 x 128, 213 of 128 x 128'),
    _c('bigM-rowk-k36', 17, 36, 64, 64, 36, 3, 3, 1, 1, 'N*P*Q = 69 632, Nc <= 64: the 128 x 64 row-k tile'),
    _c('bal16-mainks', 4, 48, 32, 32, 80, 3, 3, 1, 1, 'C % 32 != 0: the 16-wide k block with main_ks = 2 (forward)'),
    _c('bal16-mainks-dgrad', 4, 36, 32, 32, 80, 3, 3, 1, 1, 'K = 80: the 16-wide k block with main_ks = 4 (dgrad)'),
    _c('bal16-mainks-tail', 62, 80, 7, 7, 80, 3, 3, 1, 1, 'the 16-wide k block with main_ks = 4 and 8 tail slices, both directions'),
    _c('bal32-mainks-dgrad', 4, 36, 32, 32, 128, 3, 3, 1, 1, 'K = 128: main_ks = 4 without a tail in the dgrad'),
    _c('ktail-bal-tail', 1, 36, 8, 8, 500, 1, 1, 1, 0, 'KTAIL dgrad (K = 500) cut into tail slices'),
    _c('ktail-bal-tail-fwd', 1, 500, 8, 8, 48, 1, 1, 1, 0, 'KTAIL forward (C = 500) cut into tail slices'),
    _c('ktail-bal-fwd', 4, 500, 32, 32, 80, 1, 1, 1, 0, 'KTAIL forward with main_ks = 2'),
    _c('ktail-bal-both', 62, 80, 7, 7, 1000, 1, 1, 1, 0, 'KTAIL dgrad with main_ks = 4 and tail slices'),
    _c('ktail-bal16', 9, 164, 56, 56, 192, 1, 1, 1, 0, 'KTAIL on 1323 tiles of 12 k steps: the 16-wide k block, three tail slices (too few k steps for main_ks > 1)'),
    _c('taps16-ncls', 2, 32, 16, 16, 48, 3, 3, 2, 1, 'merged stride-2 dgrad with K = 48 (16-wide k block), where the header allows an addend'),
    _c('wide-pad130', 1, 16, 2, 8, 16, 1, 33, 1, 130, 'a raster wider than 32 with pad > 127: the dgrad tap table cannot hold the offsets, row-k serves it'),
    _c('bigM-3x3-mirror', 17, 64, 56, 56, 32, 3, 3, 1, 1, 'bigM-3x3 with C and K swapped: its dgrad poses that forward again'),
    _c('bal-mainks-s2', 3, 128, 64, 64, 256, 3, 3, 2, 1, 'forward of a stride-2 3x3 on 3072 pixels: main_ks = 4 under the default planner'),
    _c('bal-mainks-tail', 8, 128, 14, 14, 256, 3, 3, 1, 1, 'main_ks = 4 and tail slices in one launch (direct kernel)', {'NNL_CONV_WINO': '0'}),
    _c('wgrad-wino2d-128', 17, 128, 14, 14, 128, 3, 3, 1, 1, 'the 128-wide tile of the 2-D Winograd-domain weight gradient', {'NNL_WGRAD_WINO2D': '2'}),
    _c('kmajor', 2, 4, 2048, 2056, 4, 1, 1, 1, 0, 'N*P*Q >= 2^23: past the pixel range of the second-generation weight-gradient kernel'),
    # the (at most five) cases above 2e9 flop: tile shapes of the weight gradient that smaller problems do not reach, and the largest grids
    _c('bigM-s2', 17, 32, 112, 112, 64, 3, 3, 2, 1, 'N*P*Q = 53 312 at stride 2: merged dgrad classes on a large grid'),
    _c('bigM-200k', 17, 64, 108, 108, 64, 1, 1, 1, 0, 'N*P*Q = 198 288'),
    _c('wgrad-wino2d-kg4', 64, 128, 14, 14, 512, 3, 3, 1, 1, 'four wave groups in the 2-D Winograd-domain weight gradient: what most ResNet-34 layers take at 64 images (1.5e10 flop)'),
    _c('wgrad128x64', 64, 256, 14, 14, 512, 3, 3, 2, 1, 'ResNet-34 layer4 downsampling 3x3 at 64 images: the 128 x 64 weight-gradient tile (7.4e9 flop)'),
    _c('wgrad128x128-kg4', 64, 128, 28, 28, 512, 3, 3, 2, 1, 'the 128 x 128 weight-gradient tile with four wave groups (1.5e10 flop)'),
    _c('wgrad64x128', 16, 256, 64, 64, 64, 3, 3, 1, 1, 'N*P*Q = 65 536: the 64 x 128 weight-gradient tile, 71 splits (1.9e10 flop)', {'NNL_WGRAD_WINO': '0'}),
]
NAMED_BIG = ('wgrad-wino2d-kg4', 'wgrad128x64', 'wgrad128x128-kg4', 'wgrad64x128')       # the (at most five) cases allowed up to FLOP_CAP_NAMED


def _generated(seed=20260):
    """filter x stride x padding class, everything else drawn from the class lists by a seeded generator; a draw whose flop count passes
    3e8 is redrawn smaller (these cases are about indexing, the large-M ones are hand-written)"""
    rng = random.Random(seed)
    out = []
    rot = 0
    for (R, S) in FILTERS:
        big = max(R, S)
        for stride in STRIDES:
            for pad_class, pad in (('p0', 0), ('same', big // 2), ('full', big - 1)):
                if pad_class != 'p0' and pad == 0:
                    pad = 1                                       # 1x1: pad 1 instead of repeating pad 0
                for _ in range(200):
                    N = BATCHES[rot % len(BATCHES)] if rng.random() < 0.7 else rng.choice(BATCHES)
                    C, K = rng.choice(CHANNELS), rng.choice(CHANNELS)
                    H, W = rng.choice(SIZES), rng.choice(SIZES)
                    c = _c('g-%s' % pad_class, N, C, H, W, K, R, S, stride, pad, 'generated')
                    if valid(c) and flop(c) <= 3e8 and (H != W or rng.random() < 0.3):
                        break
                else:
                    raise AssertionError('no legal draw for %dx%d s%d p%d' % (R, S, stride, pad))
                rot += 1
                out.append(c)
    return out


GENERATED = sorted(_generated(), key=flop)
CASES = HAND + GENERATED
assert len(set(case_id(c) for c in CASES)) == len(CASES)


# ---- data and reference -----------------------------------------------------------------------------------------------------------
def int_ranges(c):
    """(a, b, bound): inputs / gradients / bias / addend from [-a, a], weights from +-{1..b}, and the largest magnitude — in units of
    the finest intermediate, 1/4 where a Winograd kernel may run — that any partial sum of any route can reach.  Ranges are narrowed
    until the bound is below 2^24 (the integers fp32 holds exactly).

    direct kernels: a dot product of `red` terms of magnitude a*b, plus bias / addend.
    Winograd F(2,3) / F(2x2,3x3) forward and dgrad (3x3 / stride 1 / pad 1 only): an input-transform entry is a signed sum of up to 4
      inputs (4a), a filter-transform entry at most 2.25 b in units of 1/4, so a Winograd-domain sum over `red` channels is at most
      9 a b red quarter-units, and the output transform adds up to 9 of those: 81 a b red.
    weight gradient: a sum over N*P*Q pixels of a*a; in the Winograd domain both transforms gain 4 per operand (16 a^2 per tile over
      N*ceil(H/2)*ceil(W/2) tiles) and the fold-back G^T dU G weighs 16 entries by at most 4 in total, in quarter-units: 256 a^2 tiles."""
    P, Q = PQ(c)
    wino = c.R == 3 and c.S == 3 and c.stride == 1 and c.pad == 1
    for a, b in ((2, 2), (1, 2), (1, 1)):
        red_f, red_d = c.C * c.R * c.S, c.K * c.R * c.S
        fwd = (81 if wino else 1) * a * b * red_f + 2 * a * (4 if wino else 1)
        dgr = (81 if wino else 1) * a * b * red_d + 2 * a * (4 if wino else 1)
        wgr = 256 * a * a * c.N * ((c.H + 1) // 2) * ((c.W + 1) // 2) if wino else a * a * c.N * P * Q
        bound = max(fwd, dgr, wgr)
        if bound < 1 << 24:
            return a, b, bound
    raise AssertionError('%s: no integer range keeps the partial sums below 2^24 (bound %d)' % (case_id(c), bound))


def make_data(c, mode, seed=0):
    """fp64 CPU tensors in torch's layouts: x [N,C,H,W], w [K,C,R,S], bias [K], dy [N,K,P,Q], add_y [N,K,P,Q] ... , add_x [N,C,H,W], pivot [K]"""
    P, Q = PQ(c)
    g = torch.Generator().manual_seed(1000 + seed)
    shapes = dict(x=(c.N, c.C, c.H, c.W), w=(c.K, c.C, c.R, c.S), bias=(c.K,), dy=(c.N, c.K, P, Q), add_x=(c.N, c.C, c.H, c.W), pivot=(c.K,))
    d = {}
    if mode == 'int':
        a, b, _ = int_ranges(c)
        for k, s in shapes.items():
            d[k] = torch.randint(-a, a + 1, s, generator=g).double()
        mag = torch.randint(1, b + 1, shapes['w'], generator=g).double()
        sign = torch.randint(0, 2, shapes['w'], generator=g).double() * 2 - 1
        d['w'] = mag * sign
    else:
        for k, s in shapes.items():
            d[k] = torch.randn(s, generator=g, dtype=torch.float64)
        d['w'] = d['w'] / (c.C * c.R * c.S) ** 0.5
        d['pivot'] = d['pivot'] * 0.1
    return d


def reference(c, d, bias=True, act=0, addend=False):
    """fp64: y = act(conv(x, w) + bias), pre = the pre-activation, dx = d(conv)/dx . dy (+ add_x), dw = d(conv)/dw . dy — the gradient
    entry points of the C ABI take dy at the convolution's output (the activation gate is the caller's)"""
    x, w = d['x'].clone().requires_grad_(True), d['w'].clone().requires_grad_(True)
    pre = F.conv2d(x, w, d['bias'] if bias else None, stride=c.stride, padding=c.pad)
    pre.backward(d['dy'])
    pre = pre.detach()
    y = torch.relu(pre) if act == 1 else torch.sigmoid(pre) if act == 2 else pre
    dx = x.grad + d['add_x'] if addend else x.grad
    return dict(y=y, pre=pre, dx=dx, dw=w.grad)


def tolerance(ref):
    """the project's per-tensor tolerance of randn mode: |got - ref| <= ATOL_REL * max|ref| + RTOL * |ref|"""
    return ATOL_REL * ref.abs().max() + RTOL * ref.abs()


def relu_excluded_share(pre, eps=1e-4):
    """share of outputs within eps of the ReLU step (two correct fp32 kernels may gate those differently)"""
    return (pre.abs() <= eps).double().mean().item()


# ---- mutants: what a kernel bug of the kind the sweep is for looks like in the reference ------------------------------------------------
def mutant_dropped_tap(c, d, ref):
    """y with one border tap removed at one output pixel: (p, q) = (0, 0), the first tap that falls INSIDE the input there.
    Returns (mutant y, index of the affected pixels)"""
    xp = F.pad(d['x'], (c.pad, c.pad, c.pad, c.pad))
    if c.pad >= c.R or c.pad >= c.S:
        return None                                               # pixel (0, 0) sees only padding
    r, s = c.pad, c.pad                                           # padded coordinates of input pixel (0, 0)
    y = ref['pre'].clone()
    y[:, :, 0, 0] -= torch.einsum('nc,kc->nk', xp[:, :, r, s], d['w'][:, :, r, s])
    return y, (slice(None), slice(None), 0, 0)


def mutant_zeroed_parity_class(c, ref):
    """dx with one parity class (h % stride, w % stride) zeroed — the first class that receives any gradient (with a 1x1 filter or a small
    input some classes receive none); stride 1: every pixel"""
    for ph in range(c.stride):
        for pw in range(c.stride):
            where = (slice(None), slice(None), slice(ph, None, c.stride), slice(pw, None, c.stride))
            if ref['dx'][where].numel() and (ref['dx'][where] != 0).double().mean() > 0.5:
                dx = ref['dx'].clone()
                dx[where] = 0
                return dx, where
    return None


def mutant_mirrored_dw(c, ref):
    """dw with the (0, 0) filter slice swapped with its mirror (R-1, S-1); None for a 1x1"""
    if c.R * c.S == 1 or torch.equal(ref['dw'][:, :, 0, 0], ref['dw'][:, :, -1, -1]):
        return None                                               # (both corner taps may see only padding: two zero slices)
    dw = ref['dw'].clone()
    dw[:, :, 0, 0], dw[:, :, -1, -1] = ref['dw'][:, :, -1, -1], ref['dw'][:, :, 0, 0]
    return dw, (slice(None), slice(None), [0, -1], [0, -1])


if __name__ == '__main__':
    tot = 0.0
    for i, c in enumerate(CASES):
        P, Q = PQ(c)
        tot += flop(c)
        print('%3d %-62s P,Q=%d,%d M=%d flop=%.2e %s%s' % (i, case_id(c), P, Q, c.N * P * Q, flop(c), c.why if c.why != 'generated' else '',
                                                            ' %s' % c.env if c.env else ''))
    print('%d cases (%d hand-written, %d generated), %.2e flop per pass over the list' % (len(CASES), len(HAND), len(GENERATED), tot))
