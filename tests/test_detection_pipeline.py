"""Detection data side: TransformBBox / get_transforms_bbox / bbox utilities / ImageDataset and ImageDataObj with 'bbox' targets,
device_data.DetectionBatches and the HIP collater (ops.detect_aug, csrc/detect_aug.hip).

The module carries a numpy RESTATEMENT of the reference's detection data path for arrays: TransformBBox.__call__
(Applications/Vision.py:559-603: lighting about the image's channel means, normalise, fliplr of image and boxes) and
AspectRatioCollater (:758-812: cv2.resize(INTER_LINEAR) by scale * rand_scale of the first sample, boxes scaled in float64, the
jitter offset, zero padding to a multiple of 32, -1 padding of boxes and categories), with the image in float64 or in an fp32 mode
with the same formulas; the boxes are float64 in both, as numpy computes them.  cv2 is not installed, so a CPU test pins the
restatement's resize to F.interpolate(mode='bilinear', align_corners=False).  The GPU tests compare the kernel's images with the
float64 restatement under tol = max(1e-6, 8 * max|restatement_fp32 - restatement_fp64|), computed per case set from the restatement
alone, and its boxes and categories with the restatement bit for bit.

What the bit-for-bit box comparison can NOT see is a multiply-add contracted into an FMA: that changes the last bit of the float64
result, and the rounding to fp32 that follows hides it in all but about one case in 2^28.  The guards against contraction are the
pragma in daug_box_f64, -ffp-contract=off on the library's build line, and tools/detect_aug_index_check.cpp, which compares the
float64 results with unfused arithmetic on cases where the two differ; a CPU test below builds and runs that program.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuralnetworklibrary_amd import device_data, ops
from neuralnetworklibrary_amd._lib import NnlError
from neuralnetworklibrary_amd.Applications import Vision as V
from test_image_pipeline import SHAPES                    # (13, 17), (17, 13), (16, 16), (9, 31), (40, 23), (5, 7)

DEV = 'cuda:0'
STATS = V.imagenet_stats
COUNTS = [0, 1, 3, 0, 2, 5]                               # boxes per image of SHAPES


# ---- the restatement ---------------------------------------------------------------------------------------------

def r_resize(img, oh, ow, dt):
    "cv2.resize(img, (ow, oh), INTER_LINEAR) for float images: half-pixel centres, two taps per axis clamped, no antialiasing"
    H, W, _ = img.shape
    fy = (np.arange(oh, dtype=dt) + dt(0.5)) * dt(H / oh) - dt(0.5)
    fx = (np.arange(ow, dtype=dt) + dt(0.5)) * dt(W / ow) - dt(0.5)
    y0, x0 = np.floor(fy).astype(int), np.floor(fx).astype(int)
    wy, wx = (fy - y0).astype(dt)[:, None, None], (fx - x0).astype(dt)[None, :, None]
    ya, yb, xa, xb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1), np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    top = img[ya][:, xa] * (1 - wx) + img[ya][:, xb] * wx
    bot = img[yb][:, xa] * (1 - wx) + img[yb][:, xb] * wx
    return (top * (1 - wy) + bot * wy).astype(dt)


def r_item(img8, target, tfm, d, dt, lit=None):
    """What TransformBBox.__call__ (Vision.py:559-603) makes of one uint8 H x W x 3 array under the draws d: (image, boxes [n, 4]
    float64, categories [n]).  Arithmetic in the reference's order: lighting about the image's own channel means, then the
    normalisation, then the mirror.  lit: a list that receives the lit, clipped, not yet normalised image."""
    x = (img8.astype(np.float32) / np.float32(255)).astype(dt)                 # open_image
    if tfm.bal_range:
        mu = x.mean(axis=(0, 1), dtype=dt)
        x = np.clip((x - mu) * dt(d['cont']) + dt(d['bal']) + mu, 0.0, 1.0).astype(dt)
        if lit is not None:
            lit.append(x)
    if tfm.stats is not None:
        mean, std = (np.asarray(v).astype(np.float32).astype(dt) for v in tfm.stats)
        x = ((x - mean) / std).astype(dt)
    mirrored = tfm.tfm_type == 'SideOn' and d['flip'] == 1
    if mirrored:
        x = x[:, ::-1]
    has_boxes = not isinstance(target, int) and len(target) > 0
    boxes = np.array([b for b, _ in target], dtype=np.float64).reshape(-1, 4) if has_boxes else np.zeros((0, 4))
    cats = np.array([c for _, c in target], dtype=np.int64) if has_boxes else np.zeros(0, dtype=np.int64)
    if mirrored and has_boxes:
        W = x.shape[1]
        boxes = np.stack([W - boxes[:, 2], boxes[:, 1], W - boxes[:, 0], boxes[:, 3]], axis=1)
    return x, boxes, cats


def r_batch(items, scales, first_draw, dt):
    """What AspectRatioCollater (Vision.py:758-812) makes of the r_item results `items` with intrinsic `scales`: every image resized
    by scale * rand_scale (r_resize for cv2.resize), boxes multiplied by scale and then by rand_scale, everything moved by the
    jitter, images zero-padded to a common multiple of 32, boxes and categories padded with -1 to the longest list (at least one
    slot).  rand_scale and the jitter are the FIRST sample's.  The order of the float64 box arithmetic is numpy's in the reference.
    Returns (images NHWC [bs, Hp, Wp, 3], boxes fp32 [bs, N, 4], cats int64 [bs, N], [(rh, rw)], (rand_scale, row_jit, col_jit))"""
    rand_scale, dy, dx = first_draw['rand_scale'], first_draw['row_jit'], first_draw['col_jit']
    shift = np.array([dx, dy, dx, dy])
    resized, moved, sizes = [], [], []
    for (x, boxes, _), scale in zip(items, scales):
        H, W = x.shape[:2]
        rh, rw = int(H * scale * rand_scale), int(W * scale * rand_scale)
        resized.append(r_resize(x, rh, rw, dt))
        sizes.append((rh, rw))
        moved.append(boxes * scale * rand_scale + shift)
    Hp = 32 * int(np.ceil(max(rh + dy for rh, _ in sizes) / 32))
    Wp = 32 * int(np.ceil(max(rw + dx for _, rw in sizes) / 32))
    N = max(1, max(len(b) for b in moved))
    images = np.zeros((len(items), Hp, Wp, 3), dtype=dt)
    out_boxes = np.full((len(items), N, 4), -1, dtype=np.float32)
    out_cats = np.full((len(items), N), -1, dtype=np.int64)
    for k, (x, b, (_, _, c)) in enumerate(zip(resized, moved, items)):
        images[k, dy:dy + x.shape[0], dx:dx + x.shape[1]] = x
        out_boxes[k, :len(b)] = b                                                # the one rounding to fp32
        out_cats[k, :len(c)] = c
    return images, out_boxes, out_cats, sizes, (rand_scale, dy, dx)


def restate(images, idx, tfm, draws, dt, lit=None):
    "the minibatch of image numbers idx under the draws, as ImageDataset.__getitem__ (:693-696) and the collater make it"
    items = [r_item(images[i]['img'], images[i]['target'], tfm, d, dt, lit) for i, d in zip(idx, draws)]
    return r_batch(items, [images[i]['scale'] for i in idx], draws[0], dt)


@pytest.mark.parametrize('H,W', [(13, 17), (9, 31), (40, 23), (5, 7)])
@pytest.mark.parametrize('factor', [0.48, 0.96, 1.7 * 1.2])
def test_restated_resize_is_torch_bilinear(H, W, factor):
    oh, ow = int(H * factor), int(W * factor)
    im = np.random.RandomState(H * 100 + W).rand(H, W, 3)
    want = F.interpolate(torch.from_numpy(im).permute(2, 0, 1)[None], size=(oh, ow), mode='bilinear', align_corners=False)
    err = np.abs(r_resize(im, oh, ow, np.float64) - want[0].permute(1, 2, 0).numpy()).max()
    print('resize %dx%d -> %dx%d: max err %.3e' % (H, W, oh, ow, err))
    assert err <= 1e-12


# ---- datasets of the tests -----------------------------------------------------------------------------------------

def _boxes(rs, H, W, n):
    "n boxes inside an H x W image with coordinates that use the whole float64 mantissa"
    out = []
    for _ in range(n):
        x0, y0 = rs.uniform(0, W - 2), rs.uniform(0, H - 2)
        out.append((np.array([x0, y0, rs.uniform(x0 + 1, W), rs.uniform(y0 + 1, H)]), int(rs.randint(0, 3))))
    return out


def _images(shapes=SHAPES, counts=COUNTS, scales=(1.0,), seed=3):
    rs = np.random.RandomState(seed)
    images = []
    for i, (H, W) in enumerate(shapes):
        img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        images.append({'img': img, 'target': _boxes(rs, H, W, counts[i % len(counts)]), 'scale': scales[i % len(scales)], 'aspect_ratio': W / H})
    return images


def _draw(row_jit=0, col_jit=0, flip=0, rand_scale=1.0, bal=None, cont=None):
    return dict(row_jit=row_jit, col_jit=col_jit, flip=flip, rand_scale=rand_scale, bal=bal, cont=cont)


# ---- CPU: TransformBBox, get_transforms_bbox, the bbox utilities ---------------------------------------------------

def _literal_draws(rs, t):
    "Vision.py:565-575, the random draws only, on RandomState rs instead of np.random"
    d = dict(bal=None, cont=None)
    d['row_jit'] = rs.randint(0, t.jitter + 1)
    d['col_jit'] = rs.randint(0, t.jitter + 1)
    d['flip'] = rs.randint(0, 2)
    d['rand_scale'] = rs.uniform(t.scale_range[0], t.scale_range[1])
    if t.bal_range:
        d['bal'] = rs.uniform(t.bal_range[0], t.bal_range[1])
        d['cont'] = rs.uniform(t.cont_range[0], t.cont_range[1])
    return d


@pytest.mark.parametrize('tfm_type', ['Basic', 'SideOn'])
@pytest.mark.parametrize('lighting', [True, False])
def test_sample_draws_in_the_reference_order(tfm_type, lighting):
    kw = {} if lighting else dict(bal_range=None, cont_range=None)
    t = V.TransformBBox(tfm_type, jitter=7, scale_range=[0.7, 1.3], **kw)
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    for _ in range(6):
        assert t.sample(a) == _literal_draws(b, t)
    assert a.randint(0, 1 << 30) == b.randint(0, 1 << 30)                           # the two streams stand at the same place


def test_get_transforms_bbox_configurations():
    ev, aug = V.get_transforms_bbox('SideOn', jitter=6, scale_range=[0.9, 1.1])
    got = lambda t: (t.tfm_type, t.bal_range, t.cont_range, t.scale_range, t.jitter, t.L, t.iter)
    assert got(ev) == ('Basic', None, None, [1, 1], 0, 100000, None)
    assert got(aug) == ('SideOn', [-0.05, 0.05], [0.95, 1.05], [0.9, 1.1], 6, 100000, None)
    assert ev.stats is V.imagenet_stats and aug.stats is V.imagenet_stats
    ev, aug = V.get_transforms_bbox('Basic')
    assert (aug.tfm_type, aug.jitter, aug.scale_range) == ('Basic', 20, [0.8, 1.2])
    assert ev.sample(np.random.RandomState(0)) == _draw()                             # the eval transform draws nothing but constants


def test_transform_bbox_rejections():
    with pytest.raises(ValueError, match='cont_range'):
        V.TransformBBox('SideOn', bal_range=[-0.1, 0.1], cont_range=None)
    with pytest.raises(ValueError, match='tfm_type'):
        V.TransformBBox('TopDown')
    t = V.TransformBBox('SideOn')
    with pytest.raises(NotImplementedError, match='DetectionBatches'):
        t(np.zeros((4, 4, 3), dtype=np.uint8), [])
    with pytest.raises(NotImplementedError, match='DetectionBatches'):
        t.get_values()


def test_get_aspect_ratio_scale():
    img = lambda H, W: np.zeros((H, W, 3), dtype=np.uint8)
    assert V.get_AspectRatioScale(img(100, 50), 200, 1000) == (0.5, 4.0)              # tall: the short side (width) goes to min_side
    assert V.get_AspectRatioScale(img(50, 100), 200, 1000) == (2.0, 4.0)              # wide
    assert V.get_AspectRatioScale(img(80, 80), 200, 1000) == (1.0, 2.5)               # square
    assert V.get_AspectRatioScale(img(100, 50), 200, 300) == (0.5, 3.0)               # max_side: 100 * 4 > 300 -> 300 / 100
    assert V.get_AspectRatioScale(img(30, 120), 60, 180) == (4.0, 1.5)
    assert V.get_AspectRatioScale(img(80, 80), 200, 100) == (1.0, 1.25)


def test_box_utilities():
    hw = np.array([3., 4., 10., 20.])
    mm = V.hw_to_mm(hw)
    assert mm.tolist() == [3., 4., 12., 23.] and V.mm_to_hw(mm).tolist() == hw.tolist()
    assert V.hw_to_mm(V.mm_to_hw(np.array([1, 2, 8, 9]))).tolist() == [1, 2, 8, 9]
    boxes, cats = V.convert_bbox_list([(np.array([1., 2., 3., 4.]), 2), (np.array([5., 6., 7., 8.]), 0)])
    assert boxes.tolist() == [[1., 2., 3., 4.], [5., 6., 7., 8.]] and cats.tolist() == [2, 0]
    padded = [torch.tensor([[1., 2., 3., 4.], [5., 6., 7., 8.], [-1., -1., -1., -1.], [9., 9., 9., 9.]]), torch.tensor([2, 0, -1, 1])]
    back = V.rev_bbox_list(padded)                                                    # stops at the FIRST -1: the slot after it is dropped too
    assert len(back) == 2 and [b.tolist() for b, _ in back] == boxes.tolist() and [int(c) for _, c in back] == [2, 0]
    assert V.rev_bbox_list([torch.full((1, 4), -1.), torch.tensor([-1])]) == []


# ---- CPU: DetectionBatches host logic, kernel call stubbed ----------------------------------------------------------

@pytest.fixture
def stub_kernel(monkeypatch):
    "ops.detect_aug replaced by a recorder: [(parameter rows, dict of the batch values)] per call, zeros out"
    calls = []

    def fake(arena, desc, image_mean, box_arena, cat_arena, params, Hp, Wp, N, row_jit, col_jit, rand_scale, stats=None):
        rows = params.numpy().view(ops.DETECT_AUG_PARAM).reshape(-1).copy()
        calls.append((rows, dict(Hp=Hp, Wp=Wp, N=N, row_jit=row_jit, col_jit=col_jit, rand_scale=rand_scale)))
        return torch.zeros(len(rows), Hp, Wp, 3), -torch.ones(len(rows), N, 4), -torch.ones(len(rows), N, dtype=torch.int64)
    monkeypatch.setattr(ops, 'detect_aug', fake)
    return calls


def _ds(images, tfm, ds_type='train'):
    return V.ImageDataset('', images, tfm, 'bbox', ds_type)


def test_detection_batches_upload(stub_kernel):
    images = _images(scales=(0.6, 1.0, 1.7))
    dl = device_data.DetectionBatches(_ds(images, V.get_transforms_bbox('SideOn')[1]), 4, grouped=True, device='cpu')
    sizes = [H * W * 3 for H, W in SHAPES]
    assert dl.arena.dtype == torch.uint8 and dl.arena.numel() == sum(sizes)
    assert dl.desc.tolist() == [[sum(sizes[:i]), H, W] for i, (H, W) in enumerate(SHAPES)]
    want_mean = np.stack([(im['img'].astype(np.int64).sum(axis=(0, 1)) / (255.0 * im['img'].shape[0] * im['img'].shape[1])).astype(np.float32)
                          for im in images])
    assert dl.image_mean.dtype == torch.float32 and np.array_equal(dl.image_mean.numpy(), want_mean)
    assert dl.box_range.tolist() == [[0, 0], [0, 1], [1, 3], [4, 0], [4, 2], [6, 5]]
    assert dl.box_arena.dtype == torch.float64 and tuple(dl.box_arena.shape) == (11, 4) and dl.cat_arena.dtype == torch.int64
    assert np.array_equal(dl.box_arena[6:].numpy(), np.stack([b for b, _ in images[5]['target']]))
    assert dl.cat_arena[1:4].tolist() == [c for _, c in images[2]['target']]
    # a test dataset has no targets whatever the images say; arenas are never empty
    test = device_data.DetectionBatches(_ds(images, V.get_transforms_bbox('SideOn')[0], 'test'), 1, grouped=False, device='cpu')
    assert test.box_range[:, 1].tolist() == [0] * 6 and tuple(test.box_arena.shape) == (1, 4)
    x, (boxes, cats) = next(iter(test))
    assert tuple(boxes.shape) == (1, 1, 4) and tuple(cats.shape) == (1, 1) and stub_kernel[-1][1]['N'] == 1


def test_detection_batches_groups(stub_kernel):
    shapes = [(10, 10), (10, 20), (8, 8), (20, 10), (12, 12), (10, 30), (6, 6)]          # aspect ratios 1, 2, 1, .5, 1, 3, 1
    images = _images(shapes)
    ds = _ds(images, V.get_transforms_bbox('SideOn')[1])
    dl = device_data.DetectionBatches(ds, 3, grouped=True, seed=5, device='cpu')
    assert [g.tolist() for g in dl.groups] == [[3, 0, 2], [4, 6, 1], [5]]                # stable under equal ratios, ragged last group
    assert len(dl) == 3 and len(device_data.DetectionBatches(ds, 2, True, world=2, device='cpu')) == 2
    epochs = []
    for e in range(3):
        del stub_kernel[:]
        shapes_seen = [tuple(x.shape) for x, _ in dl]
        epochs.append([rows['image'].tolist() for rows, _ in stub_kernel])
        assert sorted(map(sorted, epochs[-1])) == sorted(map(sorted, [g.tolist() for g in dl.groups]))   # a permutation of the groups
        assert epochs[-1] == [dl.groups[g].tolist() for g in np.random.RandomState(5 + e).permutation(3)]
        assert [s[0] for s in shapes_seen] == [len(g) for g in epochs[-1]] and dl.dp_info == (len(epochs[-1][-1]), len(epochs[-1][-1]))
    assert len({tuple(map(tuple, ep)) for ep in epochs}) > 1                             # the order changes between epochs
    first = list(stub_kernel)
    del stub_kernel[:]
    list(device_data.DetectionBatches(ds, 3, grouped=True, seed=7, device='cpu'))        # seed 7, epoch 0 == seed 5, epoch 2
    assert len(first) == len(stub_kernel)
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(first, stub_kernel))
    # not grouped (val, test): dataset order
    del stub_kernel[:]
    list(device_data.DetectionBatches(_ds(images, V.get_transforms_bbox('SideOn')[0], 'val'), 3, grouped=False, device='cpu'))
    assert [rows['image'].tolist() for rows, _ in stub_kernel] == [[0, 1, 2], [3, 4, 5], [6]]


def test_detection_batches_draws_follow_transform_sample(stub_kernel):
    tfm = V.get_transforms_bbox('SideOn', jitter=5)[1]
    images = _images(scales=(0.6, 1.0, 1.7))
    list(device_data.DetectionBatches(_ds(images, tfm), 4, grouped=True, seed=2, device='cpu'))
    rs = np.random.RandomState(2)
    order = sorted(range(6), key=lambda i: images[i]['aspect_ratio'])
    groups = [order[:4], order[4:]]
    for b, g in enumerate(rs.permutation(2)):                                            # the group permutation comes first, then the draws
        draws = [_literal_draws(rs, tfm) for _ in groups[g]]
        rows, v = stub_kernel[b]
        assert rows['image'].tolist() == groups[g]
        assert (v['rand_scale'], v['row_jit'], v['col_jit']) == (draws[0]['rand_scale'], draws[0]['row_jit'], draws[0]['col_jit'])
        assert rows['flags'].tolist() == [ops.IMAGE_AUG_FLIP * d['flip'] for d in draws]
        assert np.array_equal(rows['bal'], np.array([d['bal'] for d in draws], dtype=np.float32))
        assert np.array_equal(rows['cont'], np.array([d['cont'] for d in draws], dtype=np.float32))


TABLE_CASES = [(s, r, j) for s in range(3) for r in (0.8, 1.2) for j in ((0, 0), (3, 5), (5, 1), (2, 4))]


def _case_images(shift, counts=COUNTS):
    "SHAPES with scale {0.6, 1.0, 1.7}[(k + shift) % 3] on image k"
    scales = (0.6, 1.0, 1.7)
    return _images(scales=tuple(scales[(k + shift) % 3] for k in range(3)), counts=counts)


def _case_draws(rand_scale, jit, flip_shift=0, light=None):
    "first sample: the batch values under test; the others draw values of their own, which the collater ignores"
    bal, cont = light if light else (None, None)
    return [_draw(jit[0] if k == 0 else (k % 6), jit[1] if k == 0 else ((k + 2) % 6), (k + flip_shift) % 2,
                  rand_scale if k == 0 else 1.0 + 0.01 * k, bal, cont) for k in range(len(SHAPES))]


@pytest.mark.parametrize('shift,rand_scale,jit', TABLE_CASES)
@pytest.mark.parametrize('counts', [COUNTS, [0]], ids=['boxes', 'no_boxes'])
def test_table_equals_the_restatement(stub_kernel, shift, rand_scale, jit, counts):
    images = _case_images(shift, counts)
    tfm = V.TransformBBox('SideOn', jitter=5)
    draws = _case_draws(rand_scale, jit, light=(0.01, 1.02))
    dl = device_data.DetectionBatches(_ds(images, tfm), 6, grouped=False, device='cpu', explicit_params=lambda b, idx: draws)
    (x, (boxes, cats)), = list(dl)
    padded, rb, rc, sizes, batch_values = restate(images, range(6), tfm, draws, np.float64)
    rows, v = stub_kernel[0]
    assert list(zip(rows['rh'].tolist(), rows['rw'].tolist())) == sizes
    assert (v['Hp'], v['Wp']) == padded.shape[1:3] and v['Hp'] % 32 == 0 and v['Wp'] % 32 == 0
    assert v['N'] == rb.shape[1] == max(1, max(counts)) and (v['rand_scale'], v['row_jit'], v['col_jit']) == batch_values == (rand_scale,) + jit
    assert rows['scale'].tolist() == [im['scale'] for im in images] and rows['image'].tolist() == list(range(6))
    assert rows['box_count'].tolist() == [len(im['target']) for im in images]
    assert rows['flags'].tolist() == [ops.IMAGE_AUG_FLIP * d['flip'] for d in draws]
    assert tuple(x.shape) == (6, 3, v['Hp'], v['Wp']) and tuple(boxes.shape) == rb.shape and tuple(cats.shape) == rc.shape
    if counts == [0]:
        assert v['N'] == 1 and (rb == -1).all() and (rc == -1).all()                     # a batch without any box: one slot of -1
    # 'Basic' never flips and a transform without bal_range never lights
    del stub_kernel[:]
    basic = V.TransformBBox('Basic', None, None, jitter=5)
    list(device_data.DetectionBatches(_ds(images, basic), 6, grouped=False, device='cpu', explicit_params=lambda b, idx: draws))
    assert stub_kernel[0][0]['flags'].tolist() == [ops.IMAGE_AUG_NO_LIGHTING] * 6


def test_two_ranks_make_the_world1_minibatch(stub_kernel):
    tfm = V.get_transforms_bbox('SideOn', jitter=5)[1]
    ds = _ds(_images(SHAPES + [(8, 8)], scales=(0.6, 1.0, 1.7)), tfm)
    single = list(device_data.DetectionBatches(ds, 4, grouped=True, seed=9, device='cpu'))
    one = list(stub_kernel)
    del stub_kernel[:]
    ranks, tables = [], []
    for r in range(2):
        dl = device_data.DetectionBatches(ds, 2, grouped=True, seed=9, rank=r, world=2, device='cpu')
        assert len(dl) == len(single) == 2
        ranks.append(list(dl))
        tables.append(list(stub_kernel))
        del stub_kernel[:]
    for b in range(len(single)):
        assert np.array_equal(np.concatenate([tables[0][b][0], tables[1][b][0]]), one[b][0])      # sample for sample, draw for draw
        assert tables[0][b][1] == tables[1][b][1] == one[b][1]                                     # Hp, Wp, N, batch values: the global ones
        x = torch.cat([ranks[0][b][0], ranks[1][b][0]])
        assert x.shape == single[b][0].shape
        for part in (0, 1):
            assert torch.cat([ranks[0][b][1][part], ranks[1][b][1][part]]).shape == single[b][1][part].shape
    assert tables[0][1][0]['image'].tolist() + tables[1][1][0]['image'].tolist() == one[1][0]['image'].tolist()


def test_image_data_obj_bbox_attributes(stub_kernel):
    tfms = V.get_transforms_bbox('SideOn')
    data = V.ImageDataObj('p', 'bbox', {0: 'a', 1: 'b', 2: 'c'}, 4, tfms, _images(), _images(seed=4), num_workers=3)
    assert data.sz is None and (data.bs, data.target_type) == (4, 'bbox')
    assert data.train_ds.transform is tfms[1] and data.val_ds.transform is tfms[0] and data.train_ds.IMG_PATH == 'p/train/'
    assert isinstance(data.train_dl, device_data.DetectionBatches) and data.train_dl.grouped and data.train_dl.bs == 4
    assert isinstance(data.val_dl, device_data.DetectionBatches) and not data.val_dl.grouped and data.val_dl.bs == 1
    assert len(data.train_dl) == 2 and len(data.val_dl) == 6 and data.test_ds is None and data.test_dl is None
    list(data.val_dl)
    assert [rows['image'].tolist() for rows, _ in stub_kernel] == [[i] for i in range(6)]     # batch size 1, dataset order
    assert data.val_ds.y[2] is data.val_ds.images[2]['target'] and len(data.val_ds.y[2]) == 3
    data = V.ImageDataObj('p', 'bbox', {0: 'a'}, 4, tfms, _images(), _images(), _images(), test_name='test')
    assert data.test_ds.ds_type == 'test' and data.test_dl.bs == 1 and len(data.test_dl) == 6


def test_rejections(stub_kernel):
    tfm = V.get_transforms_bbox('SideOn')[1]
    images = _images()
    for key in ('scale', 'aspect_ratio'):
        broken = [dict(im) for im in images]
        del broken[3][key]
        with pytest.raises(ValueError, match='get_AspectRatioScale'):
            _ds(broken, tfm)
    with pytest.raises(NotImplementedError, match='bbox'):
        V.ImageDataset('', images, V.get_transforms('Basic', 8)[0], 'bbox', 'train')
    with pytest.raises(ValueError, match='TransformBBox'):
        V.ImageDataset('', images, tfm, 'single_label', 'train')
    tiny = _images(scales=(0.1,))                                                       # 5 x 7 at 0.1 * 0.8: int(0.4) == 0
    dl = device_data.DetectionBatches(_ds(tiny, tfm), 6, grouped=False, device='cpu', explicit_params=lambda b, idx: [_draw(rand_scale=0.8)] * 6)
    with pytest.raises(ValueError, match='empty side'):
        list(dl)


def test_detect_aug_refuses_cpu_tensors():
    arena = torch.zeros(6 * 5 * 3, dtype=torch.uint8)
    desc = torch.tensor([[0, 6, 5]], dtype=torch.int64)
    mean, boxes, cats = torch.zeros(1, 3), torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.int64)
    params = torch.zeros(1, ops.DETECT_AUG_PARAM.itemsize, dtype=torch.uint8)
    assert ops.DETECT_AUG_PARAM.itemsize == 48 and 'detect_aug' in ops.__all__
    with pytest.raises(NnlError):
        ops.detect_aug(arena, desc, mean, boxes, cats, params, 32, 32, 1, 0, 0, 1.0, STATS)


def test_detect_aug_c_entry_reports_bad_arguments():
    from neuralnetworklibrary_amd._lib import lib
    assert lib.nnl_detect_aug(None, 0, None, 0, None, None, None, 0, None, 1, 32, 32, 1, 0, 0, 1.0, None, None, None, None, None) == -1
    assert b'detect_aug' in lib.nnl_last_error()
    one = torch.zeros(64, dtype=torch.float64)                                           # any non-null host address: validation reads nothing
    p = one.data_ptr()
    bad = lambda **kw: lib.nnl_detect_aug(p, 64, p, 1, p, p, p, 1, p, kw.get('bs', 1), kw.get('Hp', 32), kw.get('Wp', 32), 1,
                                          kw.get('row_jit', 0), kw.get('col_jit', 0), 1.0, None, p, p, p, None)
    for kw, word in [(dict(bs=0), b'bs'), (dict(bs=65536), b'bs'), (dict(Hp=0), b'Hp'), (dict(Wp=16385), b'Wp'),
                     (dict(row_jit=-1), b'row_jit'), (dict(col_jit=-3), b'col_jit')]:
        assert bad(**kw) == -1 and word in lib.nnl_last_error() and b'detect_aug' in lib.nnl_last_error()


def test_host_walk_ends_clean_under_the_sanitizers(tmp_path):
    """tools/detect_aug_index_check.cpp, a stand-alone program: the index, pixel and box arithmetic over the tested minibatches and
    hostile rows under ASan + UBSan, and the float64 boxes against unfused arithmetic (the check that sees a contraction)"""
    import shutil
    import subprocess
    from conftest import ROOT
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'detect_aug_index_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    ROOT + '/tools/detect_aug_index_check.cpp', '-o', exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and 'clean' in run.stdout and 'differ in float64 under a fused multiply-add' in run.stdout


# ---- GPU: the kernel against the restatement --------------------------------------------------------------------------

LIGHTS = [None, (0.3, 1.5), (-0.3, 1.5)]
PRODUCT = list(itertools.product([0, 1], range(3), [0.8, 1.2], [(0, 0), (3, 5)]))        # flip shift x scale shift x rand_scale x jitter


def _run(images, tfm, draws):
    "one minibatch of all the images in dataset order through DetectionBatches with injected draws: (NHWC images, boxes, cats) as numpy"
    dl = device_data.DetectionBatches(_ds(images, tfm), len(images), grouped=False, device=DEV, explicit_params=lambda b, idx: draws)
    (x, (boxes, cats)), = list(dl)
    assert x.is_cuda and boxes.is_cuda and cats.is_cuda and ops.to_nhwc(x).data_ptr() == x.data_ptr()
    return ops.to_nhwc(x).cpu().numpy(), boxes.cpu().numpy(), cats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('stats', [STATS, None], ids=['imagenet', 'none'])
def test_gpu_minibatch_against_the_restatement(stats):
    padded_sizes, lit_all = set(), []
    for light in LIGHTS:                                                                 # one case set per lighting setting
        tfm = V.TransformBBox('SideOn', *(([-0.3, 0.3], [1.0, 1.5]) if light else (None, None)), stats=stats, jitter=5)
        results, err32 = [], 0.0
        for flip_shift, shift, rand_scale, jit in PRODUCT:
            images, draws = _case_images(shift), _case_draws(rand_scale, jit, flip_shift, light)
            got = _run(images, tfm, draws)
            r64 = restate(images, range(6), tfm, draws, np.float64, lit_all)
            r32 = restate(images, range(6), tfm, draws, np.float32)
            err32 = max(err32, np.abs(r32[0].astype(np.float64) - r64[0]).max())
            results.append((got, r64, (flip_shift, shift, rand_scale, jit)))
        tol = max(1e-6, 8 * err32)
        worst = 0.0
        for (x, boxes, cats), (padded, rb, rc, sizes, (_, row_jit, col_jit)), case in results:
            assert x.dtype == np.float32 and x.shape == padded.shape and np.isfinite(x).all(), case
            padded_sizes.update(x.shape[1:3])
            inside = np.zeros(x.shape[:3], dtype=bool)
            for k, (rh, rw) in enumerate(sizes):
                inside[k, row_jit:row_jit + rh, col_jit:col_jit + rw] = True
            assert (x[~inside] == 0.0).all() and not np.signbit(x[~inside]).any(), case   # the collater's zeros, exactly
            worst = max(worst, np.abs(x.astype(np.float64) - padded).max())
            # boxes and categories: bit for bit
            assert boxes.dtype == np.float32 and cats.dtype == np.int64 and boxes.shape == (6, 5, 4) and cats.shape == (6, 5)
            assert (boxes >= 0).sum() == 4 * sum(COUNTS) >= 44                          # 44 real coordinates per minibatch, 24 minibatches
            assert np.array_equal(boxes, rb) and np.array_equal(cats, rc), case
            for k, n in enumerate(COUNTS):
                assert (boxes[k, n:] == -1).all() and (cats[k, n:] == -1).all() and (cats[k, :n] >= 0).all()
        print('stats %s light %s: %d minibatches, kernel max err %.3e, fp32-vs-fp64 restatement tol %.3e'
              % ('imagenet' if stats is not None else 'None', light, len(results), worst, tol))
        assert worst <= tol, 'light %s: max abs err %.3e > tol %.3e' % (light, worst, tol)
    lit_all = np.concatenate([a.reshape(-1) for a in lit_all])
    assert (lit_all == 0.0).any() and (lit_all == 1.0).any()                              # both clip ends are hit
    assert {32, 64} <= padded_sizes


@pytest.mark.gpu
def test_gpu_batch_without_boxes_and_basic_transform():
    "N == 1 and everything -1; 'Basic' ignores the flip draw for image and boxes alike"
    images, draws = _case_images(1, [0]), _case_draws(1.2, (3, 5), 1, None)
    tfm = V.TransformBBox('Basic', None, None, jitter=5)
    x, boxes, cats = _run(images, tfm, draws)
    padded, rb, rc = restate(images, range(6), tfm, draws, np.float64)[:3]
    assert boxes.shape == (6, 1, 4) and (boxes == -1).all() and cats.shape == (6, 1) and (cats == -1).all() and cats.dtype == np.int64
    r32 = restate(images, range(6), tfm, draws, np.float32)[0]
    assert np.abs(x - padded).max() <= max(1e-6, 8 * np.abs(r32 - padded).max())
    images = _case_images(1)
    x, boxes, cats = _run(images, tfm, draws)
    _, rb, rc = restate(images, range(6), tfm, draws, np.float64)[:3]
    assert np.array_equal(boxes, rb) and np.array_equal(cats, rc)


@pytest.mark.gpu
def test_gpu_detect_aug_refuses_wrong_dtypes_shapes_and_layouts():
    dl = device_data.DetectionBatches(_ds(_images(), V.TransformBBox('SideOn')), 6, grouped=False, device=DEV)
    rows, v = dl._table(np.random.RandomState(0), 0, dl.groups[0])
    params = torch.from_numpy(rows.view(np.uint8).reshape(6, -1)).to(DEV)
    good = dict(arena=dl.arena, desc=dl.desc, image_mean=dl.image_mean, box_arena=dl.box_arena, cat_arena=dl.cat_arena, params=params)
    call = lambda **kw: ops.detect_aug(*[{**good, **kw}[k] for k in good], v['Hp'], v['Wp'], v['N'], v['row_jit'], v['col_jit'], v['rand_scale'], STATS)
    assert call()[0].shape == (6, v['Hp'], v['Wp'], 3)
    for kw in (dict(box_arena=dl.box_arena.float()), dict(cat_arena=dl.cat_arena.int()), dict(image_mean=dl.image_mean.double()),
               dict(arena=dl.arena.float()), dict(params=params.int()), dict(desc=dl.desc.int())):
        with pytest.raises(TypeError, match='detect_aug'):
            call(**kw)
    wide = torch.zeros(6, 64, dtype=torch.uint8, device=DEV)
    for kw in (dict(params=wide), dict(params=wide[:, :48]), dict(box_arena=dl.box_arena[:, :3].contiguous()), dict(box_arena=dl.box_arena[:0]),
               dict(cat_arena=dl.cat_arena[:-1]), dict(image_mean=dl.image_mean[:-1]), dict(desc=dl.desc[:, :2].contiguous()),
               dict(box_arena=dl.box_arena.t().contiguous().t())):
        with pytest.raises(ValueError, match='detect_aug'):
            call(**kw)


@pytest.mark.gpu
def test_gpu_minibatch_is_bitwise_repeatable():
    tfm = V.TransformBBox('SideOn', jitter=5)
    images, draws = _case_images(2), _case_draws(1.2, (3, 5), 1, (0.3, 1.5))
    a, b = _run(images, tfm, draws), _run(images, tfm, draws)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.gpu
def test_gpu_val_loader_is_the_eval_transform_in_dataset_order():
    "the ordinary path: no injection, TransformBBox.sample draws"
    images = _images(scales=(0.6, 1.0, 1.7, 2.4))
    tfms = V.get_transforms_bbox('SideOn')
    data = V.ImageDataObj('p', 'bbox', {0: 'a', 1: 'b', 2: 'c'}, 4, tfms, images, images)
    batches = list(data.val_dl)
    assert len(batches) == 6
    for i, (x, (boxes, cats)) in enumerate(batches):
        padded, rb, rc = restate(images, [i], tfms[0], [_draw()], np.float64)[:3]
        r32 = restate(images, [i], tfms[0], [_draw()], np.float32)[0]
        assert tuple(x.shape) == (1, 3) + padded.shape[1:3] and x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0
        assert x.stride()[1] == 1 and ops.to_nhwc(x).data_ptr() == x.data_ptr()           # the NHWC buffer's view, no copy
        err = np.abs(ops.to_nhwc(x).cpu().numpy() - padded).max()
        assert err <= max(1e-6, 8 * np.abs(r32 - padded).max()), 'image %d: %.3e' % (i, err)
        assert np.array_equal(boxes.cpu().numpy(), rb) and np.array_equal(cats.cpu().numpy(), rc) and cats.dtype == torch.int64
    for x, (boxes, cats) in data.train_dl:                                               # the training transform: shapes only
        assert x.shape[0] == boxes.shape[0] == cats.shape[0] and x.shape[2] % 32 == 0 and x.shape[3] % 32 == 0
        assert torch.isfinite(x).all() and boxes.shape[1] == cats.shape[1] >= 1


@pytest.mark.gpu
def test_gpu_learner_fits_retinanet_from_image_data_obj(tmp_path):
    from neuralnetworklibrary_amd.General.Core import set_default_device
    from neuralnetworklibrary_amd.General.Learner import Learner
    set_default_device(DEV)
    rs = np.random.RandomState(0)

    def mk(n):
        "tall images at scale 1, wide ones at scale 2: the aspect-ratio groups of tall images pad to 64, the others to 96 or more"
        out = []
        for i in range(n):
            H, W = (rs.randint(47, 53), rs.randint(40, 46)) if i % 2 else (rs.randint(40, 46), rs.randint(47, 53))
            img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
            target = [(np.array([4., 5., W - 6., H - 7.]), i % 3), (np.array([10., 12., 30., 33.]), (i + 1) % 3)][:1 + i % 2]
            out.append({'img': img, 'target': target, 'scale': 1.0 if H > W else 2.0, 'aspect_ratio': W / H})
        return out
    tfms = V.get_transforms_bbox('SideOn', jitter=4, scale_range=[0.9, 1.1])
    cats = {0: 'a', 1: 'b', 2: 'c'}
    data = V.ImageDataObj(str(tmp_path), 'bbox', cats, 2, tfms, mk(12), mk(6), seed=3)
    twin = V.ImageDataObj(str(tmp_path), 'bbox', cats, 2, tfms, data.train_ds.images, data.val_ds.images, seed=3)
    sizes = {tuple(x.shape[2:]) for x, _ in twin.train_dl}                               # the same seed: the epoch fit will see
    assert len(sizes) >= 2 and (64, 64) in sizes, sizes
    torch.manual_seed(0)
    verbose, Learner.verbose = Learner.verbose, False
    try:
        learner = V.ImageLearner(str(tmp_path), data, V.ObjectDetectionNet(3), optimizer='SGD_Mom', loss_func=V.SSD_loss(0.5, 0.25, 2.0))
        learner.fit(1e-3, 1, wd=1e-4)
        assert len(learner.loss_sched) == len(data.train_dl) == 6 and np.isfinite(learner.loss_sched).all()
        preds = learner.predict('val', thresh=0.0, max_boxes=5)                          # thresh 0: an untrained net still returns boxes
        assert len(preds) == len(data.val_ds) == 6
        m = learner.compute_mAP(predictions=preds, mAP_thresholds=[0.5])
    finally:
        Learner.verbose = verbose
    assert np.isfinite(m) and 0.0 <= m <= 1.0
