"""The resident image set on the GPU (csrc/image_store.hip, K16): ops.image_stats against numpy integer sums, ops.image_resize_u8
against the numpy float32 restatement of the formula in include/nnl.h, device_data.ImageStore (channel_stats, presize) and the
file-based ImageDataObj constructors end to end against the array-built objects, on the tree of golden G25."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import image_files_cases as cases
from neuralnetworklibrary_amd import device_data, ops
from neuralnetworklibrary_amd._lib import NnlError
from neuralnetworklibrary_amd.Applications import Vision as V

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARRAYS, REF_STATS, SPEC = cases.load_golden()
F32 = np.float32


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return cases.write_tree(str(tmp_path_factory.mktemp('g25')), ARRAYS, SPEC)


@pytest.fixture(autouse=True)
def _device():
    from neuralnetworklibrary_amd.General.Core import set_default_device
    from neuralnetworklibrary_amd.General.Learner import Learner
    set_default_device(DEV)
    Learner.verbose = False


# ---- restatements --------------------------------------------------------------------------------------------------

def r_resize_u8(img, oh, ow):
    "include/nnl.h, nnl_image_resize_u8, in numpy float32: every operation rounds to fp32 on its own"
    H, W, _ = img.shape
    fy = (np.arange(oh, dtype=F32) + F32(0.5)) * F32(H / oh) - F32(0.5)
    fx = (np.arange(ow, dtype=F32) + F32(0.5)) * F32(W / ow) - F32(0.5)
    y0, x0 = np.floor(fy), np.floor(fx)
    wy, wx = (fy - y0)[:, None, None], (fx - x0)[None, :, None]
    assert wy.dtype == F32 and wx.dtype == F32
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    ya, yb, xa, xb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1), np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    v = img.astype(F32)
    top = v[ya][:, xa] * (F32(1) - wx) + v[ya][:, xb] * wx
    bot = v[yb][:, xa] * (F32(1) - wx) + v[yb][:, xb] * wx
    r = top * (F32(1) - wy) + bot * wy
    assert r.dtype == F32
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def int_sums(a):
    p = a.reshape(-1, 3).astype(np.int64)
    return np.concatenate([p.sum(axis=0), (p * p).sum(axis=0)])


def pack(images, offsets, total, shift=0):
    "an arena of `total` bytes (random filler between the images) that starts `shift` bytes into its allocation, and its desc"
    buf = np.random.RandomState(9).randint(0, 256, size=shift + total).astype(np.uint8)
    desc = np.zeros((len(images), 3), dtype=np.int64)
    for k, (a, o) in enumerate(zip(images, offsets)):
        buf[shift + o:shift + o + a.size] = a.reshape(-1)
        desc[k] = (o, a.shape[0], a.shape[1])
    whole = torch.from_numpy(buf).to(DEV)
    return whole[shift:], torch.from_numpy(desc).to(DEV)


# ---- nnl_image_stats -------------------------------------------------------------------------------------------------

def stats_set():
    rs = np.random.RandomState(77)
    shapes = [(1, 1), (1, 5), (7, 1), (1, 11), (2, 3), (1, 17), (300, 257), (40, 40), (3, 3), (5, 9)]
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in shapes]
    imgs[7][:] = 255
    assert [imgs[k].size % 16 for k in (3, 4, 5)] == [1, 2, 3] and [imgs[k].size % 4 for k in (3, 4, 5)] == [1, 2, 3]
    assert imgs[6].size > 4 * ops.IMAGE_STATS_TILE_BYTES                     # several tiles: the image is split over workgroups
    offsets, o = [], 0
    for k, a in enumerate(imgs):
        o += (0, 0, 0, 1, 0, 2, 5, 0, 3, 0)[k]                                # gaps: odd and even starts, not back to back everywhere
        offsets.append(o)
        o += a.size
    assert offsets[1] % 2 == 1 and offsets[6] % 16 != 0
    return imgs, offsets, o                                                   # the last image ends exactly at arena_bytes


@pytest.mark.parametrize('shift', [0, 5])
def test_image_stats_equals_integer_sums(shift):
    imgs, offsets, total = stats_set()
    arena, desc = pack(imgs, offsets, total, shift)
    assert arena.numel() == offsets[-1] + imgs[-1].size and arena.data_ptr() % 16 == (shift % 16)
    want = np.stack([int_sums(a) for a in imgs])
    got = ops.image_stats(arena, desc)
    assert got.dtype == np.uint64 and np.array_equal(got.astype(np.int64), want)
    assert np.array_equal(ops.image_stats(arena, desc), got)                  # the same bits again
    assert np.array_equal(ops.image_stats(arena, desc, first=3, count=5).astype(np.int64), want[3:8])
    assert np.array_equal(ops.image_stats(arena, desc, first=9, count=1).astype(np.int64), want[9:])


def test_image_stats_one_large_image_alone():
    "the mean image of the arena is large: `split` is at its cap's side of the rule, and the tiles wrap over the workgroups"
    a = np.random.RandomState(3).randint(0, 256, size=(301, 199, 3)).astype(np.uint8)
    arena, desc = pack([a], [1], 1 + a.size)
    assert np.array_equal(ops.image_stats(arena, desc).astype(np.int64), int_sums(a)[None])


def test_image_stats_rejects_rows_outside_the_arena():
    """validation, not a provoked fault: the kernel checks every row against arena_bytes before it reads anything, marks a failing
    row in `out`, and ops.image_stats raises; what the host can see is refused before the launch"""
    imgs, offsets, total = stats_set()
    arena, desc = pack(imgs, offsets, total)
    for row in ([offsets[-1] + 3, 5, 9], [offsets[-1], 5, 10], [-1, 1, 1], [0, 0, 4], [0, 1 << 30, 1 << 30], [total, 1, 1]):
        bad = desc.clone()
        bad[9] = torch.tensor(row, dtype=torch.int64)
        with pytest.raises(ValueError, match='row 9'):
            ops.image_stats(arena, bad)
        assert np.array_equal(ops.image_stats(arena, bad, first=0, count=9), ops.image_stats(arena, desc, first=0, count=9))
    with pytest.raises(NnlError):
        ops.image_stats(arena, desc, first=8, count=3)
    with pytest.raises(NnlError):
        ops.image_stats(arena, desc, first=-1, count=2)
    torch.cuda.synchronize()


# ---- nnl_image_resize_u8 ---------------------------------------------------------------------------------------------

RESIZE_CASES = [((23, 17), (9, 7)), ((9, 7), (23, 17)), ((16, 9), (16, 9)), ((1, 13), (1, 5)), ((1, 13), (3, 29)), ((11, 1), (4, 1)),
                ((11, 1), (25, 2)), ((12, 20), (6, 10)), ((37, 53), (11, 50)), ((5, 7), (1, 1)), ((1, 1), (4, 6)), ((130, 170), (64, 83))]


def test_image_resize_u8_equals_the_restatement():
    rs = np.random.RandomState(21)
    srcs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for (h, w), _ in RESIZE_CASES]
    srcs[7][::2] = 255
    srcs[7][1::2] = 0                                                         # the 2x downscale: taps tie at .5, results at n + 0.5
    so, o = [], 1
    for a in srcs:
        so.append(o)
        o += a.size + 1                                                       # odd gaps
    src, sdesc = pack(srcs, so, o)
    ddesc = device_data._desc_table([d for _, d in RESIZE_CASES])[0]
    dst = ops.image_resize_u8(src, sdesc, torch.from_numpy(ddesc).to(DEV)).cpu().numpy()
    assert dst.size == int(ddesc[-1, 0] + 3 * ddesc[-1, 1] * ddesc[-1, 2])
    for a, (off, h, w) in zip(srcs, ddesc):
        got = dst[off:off + 3 * h * w].reshape(h, w, 3)
        assert np.array_equal(got, r_resize_u8(a, h, w)), (a.shape, h, w)
    off, h, w = ddesc[2]
    assert np.array_equal(dst[off:off + 3 * h * w].reshape(h, w, 3), srcs[2])  # equal sizes: the source bytes
    tie = r_resize_u8(srcs[7], 6, 10)
    assert set(np.unique(tie)) == {128}                                       # (255 + 0) / 2 = 127.5 -> 128 (ties to even)


def test_image_resize_u8_skips_invalid_rows():
    a = np.random.RandomState(1).randint(0, 256, size=(6, 5, 3)).astype(np.uint8)
    src, sdesc = pack([a, a], [0, a.size], 2 * a.size)
    ddesc = torch.tensor([[0, 3, 4], [36, 3, 5]], dtype=torch.int64, device=DEV)   # the second image would end 1 byte past dst
    dst = torch.full((36 + 44,), 7, dtype=torch.uint8, device=DEV)
    ops.image_resize_u8(src, sdesc, ddesc, dst)
    out = dst.cpu().numpy()
    assert np.array_equal(out[:36].reshape(3, 4, 3), r_resize_u8(a, 3, 4)) and (out[36:] == 7).all()


# ---- ImageStore ------------------------------------------------------------------------------------------------------

def train_files(tree):
    return [tree + '/train/' + n for n in SPEC['stats_names']], [ARRAYS['img_%02d' % i] for i in range(12)]


def exact_moments(imgs):
    "get_stats' two moments per channel as exact rationals"
    n = len(imgs)
    m = [sum(Fraction(int(int_sums(a)[c]), 255 * a.shape[0] * a.shape[1]) for a in imgs) / n for c in range(3)]
    e = [sum(Fraction(int(int_sums(a)[3 + c]), 65025 * a.shape[0] * a.shape[1]) for a in imgs) / n for c in range(3)]
    return m, e


def test_channel_stats_against_exact_arithmetic(tree):
    paths, imgs = train_files(tree)
    store = device_data.ImageStore.from_files(paths, device=DEV, threads=3, chunk_bytes=2000)
    assert np.array_equal(store.stats().astype(np.int64), np.stack([int_sums(a) for a in imgs]))
    means, stds = store.channel_stats()
    N, u = len(imgs), 2.0 ** -53
    m, e = exact_moments(imgs)
    for c in range(3):
        # N + O(1) roundings of non-negative terms: N quotients and N - 1 additions in a sum of N, one division
        assert abs(Fraction(float(means[c])) - m[c]) <= (N + 4) * u * m[c]
        var = Fraction(float(stds[c])) ** 2
        assert abs(var - (e[c] - m[c] ** 2)) <= 4 * (N + 6) * u * e[c] + 4 * u * var       # + the sqrt's own rounding, squared back
    sub = store.channel_stats([7, 2, 2])
    m, e = exact_moments([imgs[7], imgs[2], imgs[2]])
    assert all(abs(Fraction(float(sub[0][c])) - m[c]) <= 7 * u * m[c] for c in range(3))


def test_channel_stats_against_the_reference(tree):
    """G25's get_stats: the reference takes per-image float32 means of img / 255 and img^2 (numpy pairwise sums) and averages them in
    fp64, so each moment carries at most (ceil(log2(H W)) + 3) 2^-24 relative: the division by 255, the square, the pairwise adds."""
    paths, imgs = train_files(tree)
    means, stds = V.get_stats(tree + '/train', SPEC['stats_names'])
    eps = (math.ceil(math.log2(max(a.shape[0] * a.shape[1] for a in imgs))) + 3) * 2.0 ** -24
    second = stds ** 2 + means ** 2
    d_mean = np.abs(means - REF_STATS[0])
    d_std = np.abs(stds - REF_STATS[1])
    print('distance to the reference: mean', d_mean.max(), 'std', d_std.max(), 'bounds', (eps * means).min(),
          ((eps * second + 2 * eps * means ** 2) / (2 * stds)).min())
    assert (d_mean <= eps * means).all()                                      # measured: at most 4.1e-08, against bounds from 3.4e-07
    # var = E2 - m^2: |d var| <= eps E2 + 2 eps m^2, and d std = d var / (2 std)
    assert (d_std <= (eps * second + 2 * eps * means ** 2) / (2 * stds) * (1 + 1e-6)).all()       # measured: at most 8.4e-08, against bounds from 9.6e-07
    obj = V.ImageDataObj.from_csv(tree, V.get_transforms('Basic', sz=8), 4, train_csv='train.csv', val_csv='val.csv', val_name='val')
    again = obj.get_stats('train')                                            # the resident set: nothing is decoded again
    assert np.array_equal(again[0], means) and np.array_equal(again[1], stds)


def as_arrays(ds, folder):
    return [dict(im, img=cases.rgb_of(ARRAYS, SPEC, folder + '/' + im['file'])) for im in ds.images]


def test_from_csv_equals_the_array_built_object(tree):
    np.random.seed(SPEC['seeds']['csv_nohdr_suffix_split'])
    data = V.ImageDataObj.from_csv(tree, V.get_transforms('SideOn', sz=16), 4, train_csv='train_nohdr.csv', val_frac=0.25, skip_first=False,
                                   suffix='.png', seed=3)
    assert data.train_dl.arena.data_ptr() == data.val_dl.arena.data_ptr() and data.train_dl.arena.is_cuda
    twin = V.ImageDataObj(tree, 'single_label', data.categories, 4, V.get_transforms('SideOn', sz=16), as_arrays(data.train_ds, 'train'),
                          as_arrays(data.val_ds, 'train'), train_name='train', val_name='train', seed=3)
    for k in ('train_dl', 'val_dl'):
        (x, y), (xt, yt) = next(iter(getattr(data, k))), next(iter(getattr(twin, k)))
        assert x.shape[0] in (3, 4) and torch.equal(x, xt) and torch.equal(y, yt), k


def test_fit_resize_tta_from_folders(tree, tmp_path):
    np.random.seed(SPEC['seeds']['folders_split'])
    data = V.ImageDataObj.from_folders(tree, V.get_transforms('SideOn', sz=32), 3, train_name='folders', val_frac=0.3, test_name='test')
    torch.manual_seed(0)
    net = V.ImageClassificationNet(data, V.models.resnet18(), head=[[64], [0., 0.]])
    learner = V.ImageLearner(str(tmp_path), data, net)
    learner.fit(1e-3, 1)
    learner.data_resize(48, bs=3)
    assert data.train_dl.arena.data_ptr() == data.val_dl.arena.data_ptr()
    x, y = next(iter(data.train_dl))
    assert tuple(x.shape) == (3, 3, 48, 48) and torch.isfinite(x).all()
    probs, labels = learner.TTA('val')
    assert np.asarray(probs).shape == (len(data.val_ds), 3) and np.isfinite(np.asarray(probs)).all() and len(labels) == len(data.val_ds)
    probs, _ = learner.TTA('test')
    assert np.asarray(probs).shape == (2, 3)


def test_from_json_bbox_minibatch_equals_the_array_built_one(tree):
    np.random.seed(SPEC['seeds']['json_split'])
    data = V.ImageDataObj.from_json_bbox(tree, V.get_transforms_bbox('SideOn'), 3, train_json='train.json', val_frac=0.25,
                                         get_ARS=SPEC['get_ARS'], seed=2)
    twin = V.ImageDataObj(tree, 'bbox', data.categories, 3, V.get_transforms_bbox('SideOn'), as_arrays(data.train_ds, 'train'),
                          as_arrays(data.val_ds, 'train'), train_name='train', val_name='train', seed=2)
    for k in ('train_dl', 'val_dl'):
        a, b = getattr(data, k), getattr(twin, k)
        # fp32(sum / (255 H W)), quotient in fp64, on both paths: one rounding, so at most 1 ulp apart (the same expression: equal)
        ulp = np.abs(a.image_mean.cpu().numpy().view(np.int32).astype(np.int64) - b.image_mean.cpu().numpy().view(np.int32))
        assert ulp.max() <= 1
        if ulp.max() == 0:
            (x, (bx, ct)), (xt, (bxt, ctt)) = next(iter(a)), next(iter(b))
            assert torch.equal(x, xt) and torch.equal(bx, bxt) and torch.equal(ct, ctt), k
    (x, (bx, ct)), (xt, (bxt, ctt)) = next(iter(data.train_dl)), next(iter(twin.train_dl))
    assert x.shape == xt.shape and torch.equal(bx, bxt) and torch.equal(ct, ctt)            # boxes and padding do not read the means


def test_presize(tree, tmp_path):
    data = V.ImageDataObj.from_csv(tree, V.get_transforms('Basic', sz=8), 5, train_csv='train.csv', val_csv='train.csv', val_name='train',
                                   presize=8, decode_threads=2)
    store = data.val_dl.store
    assert data.train_dl.store is store
    imgs = [ARRAYS['img_%02d' % i] for i in range(12)]
    want_shapes = []
    for a in imgs:
        H, W = a.shape[:2]
        if min(H, W) <= 8:
            want_shapes.append((H, W))                                        # small images are stored as they are
        else:
            want_shapes.append((8, int(W * 8 / H)) if H <= W else (int(H * 8 / W), 8))
    assert store.shapes == want_shapes and store.orig_shapes == [a.shape[:2] for a in imgs]
    assert sum(s != o for s, o in zip(store.shapes, store.orig_shapes)) >= 6
    small = [r_resize_u8(a, h, w) for a, (h, w) in zip(imgs, want_shapes)]
    for k, (a, s) in enumerate(zip(imgs, small)):
        assert np.array_equal(store[k].numpy(), s)
        if s.shape == a.shape:
            assert np.array_equal(s, a)
    twin = device_data.ImageBatches(V.ImageDataset('', [dict(im, img=s) for im, s in zip(data.val_ds.images, small)],
                                                   V.get_transforms('Basic', sz=8)[0], 'single_label', 'val'), 5, False)
    for (x, y), (xt, yt) in zip(data.val_dl, twin):
        assert torch.equal(x, xt) and torch.equal(y, yt)
    # the fixed-size form, and save_resized, which enlarges
    fixed = device_data.ImageStore.from_files([tree + '/train/img00.png', tree + '/train/img01.png'], presize=(6, 9))
    assert fixed.shapes == [(6, 9)] * 2 and np.array_equal(fixed[1].numpy(), r_resize_u8(imgs[1], 6, 9))
    V.save_resized(tree + '/test', str(tmp_path / 'small'), 10)
    for name, key in (('t0.png', 'img_02'), ('t1.png', 'img_09')):
        a = ARRAYS[key]
        H, W = a.shape[:2]
        h, w = (10, int(W * 10 / H)) if H <= W else (int(H * 10 / W), 10)
        assert np.array_equal(V.open_image_u8(str(tmp_path / 'small' / name)), r_resize_u8(a, h, w))
