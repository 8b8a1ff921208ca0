"""Vision data side: Transform / get_transforms / ImageDataset / ImageDataObj, device_data.ImageBatches and the HIP augmenter
(ops.image_aug, csrc/image_aug.hip).

The module carries a numpy RESTATEMENT of the reference's classification transform for arrays (Transform.__call__,
Applications/Vision.py:449-507: crop, cv2.resize(INTER_LINEAR), cv2.warpAffine(BORDER_REFLECT), fliplr, rot90, lighting,
normalise), in float64 and in an fp32 mode with the same formulas.  cv2 is not installed, so the CPU tests pin the restatement's
resize and warp to independent torch CPU ops (F.interpolate, F.grid_sample); the GPU tests compare the kernel with the float64
restatement under tol = max(1e-6, 8 * max|restatement_fp32 - restatement_fp64|), computed per case set from the restatement alone.
Known difference from cv2: warpAffine rounds source coordinates to 1/32 pixel, the restatement and the kernel do not.
"""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuralnetworklibrary_amd import device_data, ops
from neuralnetworklibrary_amd._lib import NnlError
from neuralnetworklibrary_amd.Applications import Vision as V

DEV = 'cuda:0'
STATS = V.imagenet_stats


# ---- the restatement ---------------------------------------------------------------------------------------------

def r_reflect(i, n):
    "cv2 BORDER_REFLECT fedcba|abcdefgh|hgfedcb, any distance"
    p = 2 * n
    i = np.mod(i, p)
    return np.where(i >= n, p - 1 - i, i)


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


def r_inverse_map(H, W, deg, zoom, dt):
    "inverse of cv2.getRotationMatrix2D((W // 2, H // 2), deg, zoom), float64, rounded to dt"
    a, b = zoom * math.cos(math.radians(deg)), zoom * math.sin(math.radians(deg))
    cx, cy = W // 2, H // 2
    M = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy], [0, 0, 1]], dtype=np.float64)
    return np.linalg.inv(M).astype(dt)


def r_warp_coords(H, W, Mi, dt):
    ys, xs = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing='ij')
    sx = (Mi[0, 0] * xs + Mi[0, 1] * ys + Mi[0, 2]).astype(dt)
    sy = (Mi[1, 0] * xs + Mi[1, 1] * ys + Mi[1, 2]).astype(dt)
    return sx, sy


def r_warp(img, deg, zoom, dt):
    "cv2.warpAffine(img, getRotationMatrix2D(centre, deg, zoom), (W, H), borderMode=BORDER_REFLECT), bilinear, exact coordinates"
    H, W, _ = img.shape
    sx, sy = r_warp_coords(H, W, r_inverse_map(H, W, deg, zoom, dt), dt)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    wx, wy = (sx - x0).astype(dt)[..., None], (sy - y0).astype(dt)[..., None]
    xa, xb, ya, yb = r_reflect(x0, W), r_reflect(x0 + 1, W), r_reflect(y0, H), r_reflect(y0 + 1, H)
    out = (img[ya, xa] * (1 - wx) + img[ya, xb] * wx) * (1 - wy) + (img[yb, xa] * (1 - wx) + img[yb, xb] * wx) * wy
    return out.astype(dt)


def r_crop(img, crop_type, origin):
    "Vision.py:469-481; origin: the value the reference draws for crop_type 'random'"
    rows, cols = img.shape[0], img.shape[1]
    L = min(rows, cols)
    if crop_type is None:
        return img
    if rows > L:
        r = {'center': (rows - L) // 2, 'random': origin}.get(crop_type) if isinstance(crop_type, str) else int((rows - L) * crop_type)
        return img[r:r + L, :]
    if cols > L:
        c = {'center': (cols - L) // 2, 'random': origin}.get(crop_type) if isinstance(crop_type, str) else int((cols - L) * crop_type)
        return img[:, c:c + L]
    return img


def restate(img8, sz, crop_type, dt, origin=None, deg=None, zoom=None, flip=0, rot=0, bal=None, cont=None, stats=None,
            prelight=None):
    """Transform.__call__ (Vision.py:449-507) on a uint8 H x W x 3 array with given draws; deg None: no rotate-zoom, bal None: no
    lighting.  prelight: a list that receives the lit, clipped, not yet normalised image."""
    img = (img8.astype(np.float32) / np.float32(255)).astype(dt)              # open_image
    img = r_crop(img, crop_type, origin)
    img = r_resize(img, sz[0], sz[1], dt)
    if deg is not None:
        img = r_warp(img, deg, zoom, dt)
    if flip:
        img = np.fliplr(img)
    img = np.rot90(img, rot)
    if bal is not None:
        mu = img.mean(axis=(0, 1), dtype=dt)
        img = np.clip((img - mu) * dt(cont) + dt(bal) + mu, 0.0, 1.0)
    if prelight is not None:
        prelight.append(img)
    if stats is not None:
        img = (img - stats[0].astype(np.float32).astype(dt)) / stats[1].astype(np.float32).astype(dt)
    return np.ascontiguousarray(img).astype(dt)


# ---- CPU: the restatement against independent torch ops ----------------------------------------------------------

@pytest.mark.parametrize('H,W', [(13, 17), (9, 31), (16, 16), (40, 23)])
@pytest.mark.parametrize('o', [8, 12, (8, 12)])
def test_restated_resize_is_torch_bilinear(H, W, o):
    oh, ow = (o, o) if isinstance(o, int) else o
    im = np.random.RandomState(H * 100 + W).rand(H, W, 3)
    want = F.interpolate(torch.from_numpy(im).permute(2, 0, 1)[None], size=(oh, ow), mode='bilinear', align_corners=False)
    err = np.abs(r_resize(im, oh, ow, np.float64) - want[0].permute(1, 2, 0).numpy()).max()
    print('resize %dx%d -> %dx%d: max err %.3e' % (H, W, oh, ow, err))
    assert err <= 1e-12


@pytest.mark.parametrize('S,deg,zoom', [(8, 10., 1.05), (12, -10., 1.0), (12, 37., 1.3), (8, 170., 1.0)])
def test_restated_warp_is_torch_grid_sample_reflection(S, deg, zoom):
    im = np.random.RandomState(S).rand(S, S, 3)
    sx, sy = r_warp_coords(S, S, r_inverse_map(S, S, deg, zoom, np.float64), np.float64)
    grid = torch.from_numpy(np.stack([(2 * sx + 1) / S - 1, (2 * sy + 1) / S - 1], -1))[None]
    want = F.grid_sample(torch.from_numpy(im).permute(2, 0, 1)[None], grid, mode='bilinear', padding_mode='reflection', align_corners=False)
    err = np.abs(r_warp(im, deg, zoom, np.float64) - want[0].permute(1, 2, 0).numpy()).max()
    print('warp %d, %g deg, zoom %g: max err %.3e' % (S, deg, zoom, err))
    assert err <= 1e-12


# ---- CPU: Transform, get_transforms, argument rejection -----------------------------------------------------------

def _literal_draws(rs, t, rows, cols):
    "Vision.py:452-481, the random draws only, on RandomState rs instead of np.random"
    d = dict(deg=None, zoom=None, bal=None, cont=None, origin=None)
    d['flip'] = rs.randint(0, 2)
    d['rot'] = rs.randint(0, 4)
    if t.max_deg: d['deg'] = rs.uniform(-t.max_deg, t.max_deg)
    if t.max_zoom: d['zoom'] = rs.uniform(1, t.max_zoom)
    if t.bal_range: d['bal'] = rs.uniform(t.bal_range[0], t.bal_range[1])
    if t.cont_range: d['cont'] = rs.uniform(t.cont_range[0], t.cont_range[1])
    L = min(rows, cols)
    if t.crop_type is None:
        pass
    elif rows > L:
        if t.crop_type == 'random': d['origin'] = rs.randint(0, rows - L + 1)
    elif cols > L:
        if t.crop_type == 'random': d['origin'] = rs.randint(0, cols - L + 1)
    return d


@pytest.mark.parametrize('tfm_type', ['Basic', 'SideOn', 'TopDown'])
@pytest.mark.parametrize('ranges', ['set', 'none', 'zoom_only'])
@pytest.mark.parametrize('crop_type', ['random', 'center', 0.25, None])
def test_sample_draws_in_the_reference_order(tfm_type, ranges, crop_type):
    kw = {'set': {}, 'none': dict(max_deg=None, max_zoom=None, bal_range=None, cont_range=None),
          'zoom_only': dict(max_deg=None, max_zoom=1.2, bal_range=None, cont_range=[0.9, 1.1])}[ranges]
    t = V.Transform(tfm_type, crop_type, sz=16, **kw)
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    for H, W in [(40, 23), (23, 40), (16, 16), (9, 31), (31, 9), (5, 5)]:          # tall, wide, square
        assert t.sample(a, H, W) == _literal_draws(b, t, H, W)
    assert a.randint(0, 1 << 30) == b.randint(0, 1 << 30)                           # the two streams stand at the same place


def test_get_transforms_configurations():
    ev, aug = V.get_transforms('SideOn', sz=64, stats=V.alternate_stats)
    got = lambda t: (t.tfm_type, t.crop_type, t.pad, t.sz, t.max_deg, t.max_zoom, t.bal_range, t.cont_range, t.max_noise)
    assert got(ev) == ('Basic', 'center', None, (64, 64), None, None, None, None, None)
    assert got(aug) == ('SideOn', 'random', None, (64, 64), 10, 1.05, [-0.05, 0.05], [0.95, 1.05], None)
    assert ev.stats is V.alternate_stats and aug.stats is V.alternate_stats
    assert V.get_transforms('Basic')[0].sz == (224, 224) and V.get_transforms('Basic')[1].stats is V.imagenet_stats


def test_param_row_follows_the_reference_switches():
    t = V.Transform('SideOn', 0.7, sz=(8, 12))
    row = t.param_row(3, 40, 23, flip=1, rot=2, deg=10., zoom=1.05, bal=0.01, cont=1.02)
    assert (row['image'], row['crop_y'], row['crop_x'], row['crop_h'], row['crop_w']) == (3, int(17 * 0.7), 0, 23, 23)
    assert row['flags'] == ops.IMAGE_AUG_FLIP and row['rot'] == 0                     # rot counts for 'TopDown' only
    assert np.abs(row['m'] - r_inverse_map(8, 12, 10., 1.05, np.float64)[:2].reshape(6)).max() <= 1e-6      # fp32 rounding of |m| < 8
    ev = V.get_transforms('TopDown', 8)[0]
    row = ev.param_row(0, 9, 31, flip=1, rot=3)
    assert row['flags'] == ops.IMAGE_AUG_NO_WARP | ops.IMAGE_AUG_NO_LIGHTING and row['rot'] == 0
    assert (row['crop_y'], row['crop_x'], row['crop_h'], row['crop_w']) == (0, 11, 9, 9)
    assert V.Transform('Basic', None, sz=8).param_row(0, 9, 31)[['crop_y', 'crop_x', 'crop_h', 'crop_w']].tolist() == (0, 0, 9, 31)
    assert ops.IMAGE_AUG_PARAM.itemsize == 64


def _img(H=6, W=5, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def test_argument_rejection():
    with pytest.raises(NotImplementedError, match='pad'):
        V.Transform('Basic', 'center', pad=4)
    with pytest.raises(NotImplementedError, match='max_noise'):
        V.Transform('Basic', 'center', max_noise=0.1)
    with pytest.raises(NotImplementedError, match='sz'):
        V.Transform('Basic', 'center', sz=None)
    with pytest.raises(ValueError, match='max_zoom'):
        V.Transform('Basic', 'center', max_deg=10, max_zoom=None)
    with pytest.raises(ValueError, match='square'):
        V.Transform('TopDown', 'center', sz=(8, 12))
    with pytest.raises(NotImplementedError, match='ImageBatches'):
        V.Transform('Basic', 'center')(_img())
    tfm = V.get_transforms('Basic', 8)[0]
    with pytest.raises(NotImplementedError, match='file name'):
        V.ImageDataset('x/', [{'img': 'dog.png', 'target': 0}], tfm, 'single_label', 'train')
    with pytest.raises(NotImplementedError, match='bbox'):
        V.ImageDataset('x/', [{'img': _img(), 'target': []}], tfm, 'bbox', 'train')
    ds = V.ImageDataset('x/', [{'img': _img(), 'target': 1}], tfm, 'single_label', 'train')
    assert (ds.IMG_PATH, ds.transform, ds.target_type, ds.ds_type, ds.y, len(ds)) == ('x/', tfm, 'single_label', 'train', [1], 1)


def test_image_aug_refuses_cpu_tensors():
    arena = torch.zeros(6 * 5 * 3, dtype=torch.uint8)
    desc = torch.tensor([[0, 6, 5]], dtype=torch.int64)
    params = torch.zeros(1, 64, dtype=torch.uint8)
    with pytest.raises(NnlError):
        ops.image_aug(arena, desc, params, (8, 8), STATS, lighting=True)


def test_image_aug_c_entry_reports_bad_arguments():
    from neuralnetworklibrary_amd._lib import lib
    assert lib.nnl_image_aug(None, 0, None, 0, None, 1, 8, 8, None, 0, None, None, 0, None) == -1
    assert b'image_aug' in lib.nnl_last_error()
    assert lib.nnl_image_aug_workspace_bytes(64, 224, 224) == 64 * 196 * 3 * 4
    assert lib.nnl_image_aug_workspace_bytes(0, 8, 8) == 0


# ---- CPU: ImageBatches host logic, kernel call stubbed -----------------------------------------------------------

SHAPES = [(13, 17), (17, 13), (16, 16), (9, 31), (40, 23), (5, 7)]          # the odd-sized one last: the arena ends on it


def _images(shapes=SHAPES, seed=3, target=lambda i: i):
    rs = np.random.RandomState(seed)
    return [{'img': rs.randint(0, 256, (H, W, 3)).astype(np.uint8), 'target': target(i)} for i, (H, W) in enumerate(shapes)]


@pytest.fixture
def stub_kernel(monkeypatch):
    "ops.image_aug replaced by a recorder: [(image numbers, parameter rows)] per call, zeros out"
    calls = []

    def fake(arena, desc, params, sz, stats=None, lighting=False):
        rows = params.numpy().view(ops.IMAGE_AUG_PARAM).reshape(-1).copy()
        calls.append(rows)
        return torch.zeros(len(rows), sz[0], sz[1], 3)
    monkeypatch.setattr(ops, 'image_aug', fake)
    return calls


def _ds7(tfm):
    return V.ImageDataset('', _images(SHAPES + [(8, 8)]), tfm, 'single_label', 'train')


def test_image_batches_len_ragged_tail_and_upload(stub_kernel):
    ds = _ds7(V.get_transforms('TopDown', 8)[1])
    dl = device_data.ImageBatches(ds, 3, shuffle=False, device='cpu')
    assert len(dl) == 3 and len(device_data.ImageBatches(ds, 3, False, world=2, device='cpu')) == 2
    batches = list(dl)
    assert [tuple(x.shape) for x, _ in batches] == [(3, 3, 8, 8), (3, 3, 8, 8), (1, 3, 8, 8)]
    assert torch.cat([y for _, y in batches]).tolist() == list(range(7)) and batches[0][1].dtype == torch.int64
    assert dl.dp_info == (1, 1)
    sizes = [H * W * 3 for H, W in SHAPES + [(8, 8)]]
    assert dl.arena.dtype == torch.uint8 and dl.arena.numel() == sum(sizes)
    assert dl.desc.tolist() == [[sum(sizes[:i]), H, W] for i, (H, W) in enumerate(SHAPES + [(8, 8)])]
    assert np.array_equal(dl.arena[dl.desc[5, 0]:dl.desc[6, 0]].numpy(), ds.images[5]['img'].reshape(-1))


def test_image_batches_permutation_per_epoch(stub_kernel):
    ds = _ds7(V.get_transforms('TopDown', 8)[1])
    dl = device_data.ImageBatches(ds, 3, shuffle=True, seed=5, device='cpu')
    e0 = torch.cat([y for _, y in dl]).tolist()
    e1 = torch.cat([y for _, y in dl]).tolist()
    assert sorted(e0) == list(range(7)) and sorted(e1) == list(range(7)) and e0 != e1
    assert e0 == np.random.RandomState(5).permutation(7).tolist() and e1 == np.random.RandomState(6).permutation(7).tolist()
    n_calls = len(stub_kernel)
    again = device_data.ImageBatches(ds, 3, shuffle=True, seed=5, device='cpu')
    assert torch.cat([y for _, y in again]).tolist() == e0                       # the same seed: the same order and the same draws
    first, second = stub_kernel[:3], stub_kernel[n_calls:n_calls + 3]
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert [int(i) for rows in first for i in rows['image']] == e0               # the table's image numbers are the permutation


def test_image_batches_draws_follow_transform_sample(stub_kernel):
    tfm = V.get_transforms('TopDown', 8)[1]
    ds = _ds7(tfm)
    list(device_data.ImageBatches(ds, 3, shuffle=True, seed=2, device='cpu'))
    rs = np.random.RandomState(2)
    perm = rs.permutation(7)
    want = [tfm.param_row(i, *ds.images[i]['img'].shape[:2], **tfm.sample(rs, *ds.images[i]['img'].shape[:2])) for i in perm]
    assert np.array_equal(np.concatenate(stub_kernel), np.stack(want))


def test_image_batches_two_ranks_make_the_world1_minibatch(stub_kernel):
    ds = _ds7(V.get_transforms('SideOn', 8)[1])
    single = list(device_data.ImageBatches(ds, 4, shuffle=True, seed=9, device='cpu'))
    one = list(stub_kernel)
    del stub_kernel[:]
    ranks, tables = [], []
    for r in range(2):
        dl = device_data.ImageBatches(ds, 2, shuffle=True, seed=9, rank=r, world=2, device='cpu')
        assert len(dl) == len(single)
        ranks.append(list(dl))
        tables.append(list(stub_kernel))
        del stub_kernel[:]
    for b in range(len(single)):
        assert torch.equal(torch.cat([ranks[0][b][1], ranks[1][b][1]]), single[b][1])
        assert np.array_equal(np.concatenate([tables[0][b], tables[1][b]]), one[b])      # sample for sample, draw for draw


def test_image_batches_targets_and_explicit_params(stub_kernel):
    tfm = V.get_transforms('Basic', 8)[0]
    multi = V.ImageDataset('', _images(target=lambda i: np.array([i % 2, 1, 0])), tfm, 'multi_label', 'val')
    y = next(iter(device_data.ImageBatches(multi, 4, False, device='cpu')))[1]
    assert y.dtype == torch.float32 and y.tolist() == [[0, 1, 0], [1, 1, 0], [0, 1, 0], [1, 1, 0]]
    test = V.ImageDataset('', _images(target=lambda i: 0), tfm, 'single_label', 'test')
    y = next(iter(device_data.ImageBatches(test, 4, False, device='cpu')))[1]
    assert y.dtype == torch.int64 and y.tolist() == [0, 0, 0, 0]
    seen = []

    def inject(b, idx):
        seen.append((b, list(idx)))
        return np.stack([tfm.param_row(i, *SHAPES[i]) for i in idx])
    list(device_data.ImageBatches(test, 4, False, device='cpu', explicit_params=inject))
    assert seen == [(0, [0, 1, 2, 3]), (1, [4, 5])]


def test_image_data_obj_attributes(stub_kernel):
    tfms = V.get_transforms('SideOn', (8, 12))
    data = V.ImageDataObj('p', 'single_label', {0: 'a', 1: 'b'}, 4, tfms, _images(), _images(seed=4), num_workers=3)
    assert (data.sz, data.bs, data.target_type, data.categories) == ((8, 12), 4, 'single_label', {0: 'a', 1: 'b'})
    assert data.train_ds.transform is tfms[1] and data.val_ds.transform is tfms[0] and data.train_ds.IMG_PATH == 'p/train/'
    assert data.test_ds is None and data.test_dl is None
    assert isinstance(data.train_dl, device_data.ImageBatches) and data.train_dl.shuffle and not data.val_dl.shuffle
    data = V.ImageDataObj('p', 'single_label', {0: 'a'}, 4, tfms, _images(), _images(), _images(), test_name='test')
    assert data.test_ds.ds_type == 'test' and len(data.test_dl) == 2 and data.test_ds.IMG_PATH == 'p/test/'


# ---- GPU: the kernel against the float64 restatement --------------------------------------------------------------

def _run(tfm, cases, images):
    """One minibatch of `cases` = [(image number, crop_type, draws)] through ImageBatches with injected rows, against the
    restatement: sample k of the dataset is the image that case k names.  Returns (kernel output NHWC numpy, fp64 restatement,
    tol, lit images of the restatement)."""
    ds = V.ImageDataset('', [{'img': images[i]['img'], 'target': i} for i, _, _ in cases], tfm, 'single_label', 'val')
    sz, stats = tfm.sz, tfm.stats
    kw = dict(tfm_type=tfm.tfm_type, sz=sz, max_deg=tfm.max_deg, max_zoom=tfm.max_zoom, bal_range=tfm.bal_range,
              cont_range=tfm.cont_range, stats=stats)

    def inject(b, idx):
        assert b == 0 and list(idx) == list(range(len(cases)))
        return np.stack([V.Transform(crop_type=crop, **kw).param_row(k, *images[i]['img'].shape[:2], **draws)
                         for k, (i, crop, draws) in enumerate(cases)])
    (x, y), = list(device_data.ImageBatches(ds, len(cases), False, device=DEV, explicit_params=inject))
    assert y.tolist() == [i for i, _, _ in cases]
    got = ops.to_nhwc(x).cpu().numpy()
    lit = []

    def ref(dt):
        out = []
        for i, crop, d in cases:
            eff = dict(d)
            if tfm.tfm_type == 'Basic': eff['flip'] = 0
            if tfm.tfm_type != 'TopDown': eff['rot'] = 0
            if not tfm.max_deg: eff['deg'] = eff['zoom'] = None
            if not tfm.bal_range: eff['bal'] = eff['cont'] = None
            out.append(restate(images[i]['img'], sz, crop, dt, stats=stats, prelight=lit if dt is np.float64 else None, **eff))
        return np.stack(out).astype(np.float64)
    r64, r32 = ref(np.float64), ref(np.float32)
    tol = max(1e-6, 8 * np.abs(r32 - r64).max())
    return got, r64, tol, lit


def _check(name, got, r64, tol):
    assert got.shape == r64.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - r64).max()
    print('%s: %d samples, kernel max err %.3e, fp32-vs-fp64 restatement tol %.3e' % (name, len(got), err, tol))
    assert err <= tol, '%s: max abs err %.3e > tol %.3e' % (name, err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('sz', [8, (8, 12)])
def test_gpu_eval_transform(sz):
    tfm = V.get_transforms('SideOn', sz)[0]
    images = _images()
    cases = [(i, 'center', dict(flip=1, rot=3)) for i in range(len(images))]     # 'Basic': the draws are made and ignored
    got, r64, tol, _ = _run(tfm, cases, images)
    _check('eval sz %s' % (sz,), got, r64, tol)
    # and through the ordinary path (Transform.sample draws, no injection)
    ds = V.ImageDataset('', images, tfm, 'single_label', 'val')
    x = torch.cat([ops.to_nhwc(xb) for xb, _ in device_data.ImageBatches(ds, 4, False, device=DEV)])
    assert np.array_equal(x.cpu().numpy(), got)


CROPS = ['center', 0.25, 0.7, None, 'random']


def _train_cases():
    cases = []
    for k, (flip, rot, deg, zoom) in enumerate(itertools.product([0, 1], range(4), [-10., 10., 37., 170.], [1.0, 1.05, 1.3])):
        i, crop = k % len(SHAPES), CROPS[k % len(CROPS)]
        bal, cont = [(0.3, 1.5), (-0.3, 1.5), (0.02, 0.97)][k % 3]
        H, W = SHAPES[i]
        cases.append((i, crop, dict(flip=flip, rot=rot, deg=deg, zoom=zoom, bal=bal, cont=cont, origin=(k * 5) % (abs(H - W) + 1))))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize('sz,stats', [(8, STATS), (12, STATS), (16, STATS), (12, None)])
def test_gpu_training_transform(sz, stats):
    tfm = V.Transform('TopDown', 'random', sz=sz, stats=stats)
    got, r64, tol, lit = _run(tfm, _train_cases(), _images())
    lit = np.stack(lit)
    assert (lit == 0.0).any() and (lit == 1.0).any()                              # both clip ends are hit
    _check('train sz %d stats %s' % (sz, 'imagenet' if stats is not None else 'None'), got, r64, tol)


@pytest.mark.gpu
def test_gpu_training_transform_side_on_non_square_and_no_lighting():
    "the switches of Vision.py:487-496 one at a time: LR-flip on a non-square sz, rotate-zoom without lighting, lighting alone"
    images = _images()
    draws = [dict(flip=k % 2, rot=k % 4, deg=[-10., 37.][k % 2], zoom=1.05, bal=0.3, cont=1.5, origin=k % 3) for k in range(12)]
    cases = [(k % len(SHAPES), CROPS[k % len(CROPS)], d) for k, d in enumerate(draws)]
    for name, tfm in [('SideOn 8x12', V.Transform('SideOn', 'random', sz=(8, 12))),
                      ('warp only', V.Transform('TopDown', 'random', sz=12, bal_range=None, cont_range=None)),
                      ('lighting only', V.Transform('SideOn', 'random', sz=12, max_deg=None, max_zoom=None, stats=None))]:
        got, r64, tol, _ = _run(tfm, cases, images)
        _check(name, got, r64, tol)


@pytest.mark.gpu
def test_gpu_training_transform_is_bitwise_repeatable():
    tfm = V.Transform('TopDown', 'random', sz=16)
    a = _run(tfm, _train_cases(), _images())[0]
    b = _run(tfm, _train_cases(), _images())[0]
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_gpu_image_data_obj_end_to_end():
    shapes = SHAPES + [(8, 8)]
    tfms = V.get_transforms('TopDown', 8)
    train = _images(shapes)
    val = _images(shapes, seed=8, target=lambda i: (i * 3) % 7)
    data = V.ImageDataObj('p', 'single_label', {i: str(i) for i in range(7)}, 3, tfms, train, val, seed=4)
    for epoch in range(2):
        batches = list(data.train_dl)
        assert [tuple(x.shape) for x, _ in batches] == [(3, 3, 8, 8), (3, 3, 8, 8), (1, 3, 8, 8)]              # ragged last batch
        assert torch.cat([y for _, y in batches]).tolist() == np.random.RandomState(4 + epoch).permutation(7).tolist()
        for x, y in batches:
            assert x.is_cuda and x.dtype == torch.float32 and y.dtype == torch.int64 and y.is_cuda
            assert x.is_contiguous(memory_format=torch.channels_last) or x.shape[0] == 1
            assert x.stride()[1] == 1 and ops.to_nhwc(x).data_ptr() == x.data_ptr()                             # no copy
            assert torch.isfinite(x).all()
    first = [(x.clone(), y.clone()) for x, y in data.val_dl]
    second = list(data.val_dl)
    assert torch.cat([y for _, y in first]).tolist() == [(i * 3) % 7 for i in range(7)]
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(first, second))
    # the val loader is the eval transform of each image, in order
    want, want32 = [np.stack([restate(im['img'], (8, 8), 'center', dt, stats=STATS) for im in val]) for dt in (np.float64, np.float32)]
    _check('val_dl', torch.cat([ops.to_nhwc(x) for x, _ in first]).cpu().numpy(), want, max(1e-6, 8 * np.abs(want32 - want).max()))

    multi = V.ImageDataObj('p', 'multi_label', {0: 'a', 1: 'b', 2: 'c'}, 4, tfms, _images(target=lambda i: np.array([i % 2, 1, 0])),
                           _images(target=lambda i: np.array([0, 0, 1])), _images(target=lambda i: 0), test_name='test')
    x, y = next(iter(multi.val_dl))
    assert y.dtype == torch.float32 and y.tolist() == [[0, 0, 1]] * 4 and tuple(x.shape) == (4, 3, 8, 8)
    ys = torch.cat([y for _, y in multi.train_dl])
    assert tuple(ys.shape) == (6, 3) and ys[:, 0].sum().item() == 3 and ys[:, 1].tolist() == [1.] * 6
    assert [y.tolist() for _, y in multi.test_dl] == [[0] * 4, [0] * 2]


@pytest.mark.gpu
def test_gpu_learner_fits_resnet18_from_image_data_obj(tmp_path):
    from neuralnetworklibrary_amd.General.Learner import Learner
    rs = np.random.RandomState(0)
    mk = lambda n: [{'img': rs.randint(0, 256, (rs.randint(33, 48), rs.randint(33, 48), 3)).astype(np.uint8), 'target': i % 3}
                    for i in range(n)]
    data = V.ImageDataObj(str(tmp_path), 'single_label', {0: 'a', 1: 'b', 2: 'c'}, 8, V.get_transforms('SideOn', 32), mk(24), mk(12))
    torch.manual_seed(0)
    verbose, Learner.verbose = Learner.verbose, False
    try:
        learner = Learner(str(tmp_path), data, V.ImageClassificationNet(data, V.models.resnet18()))
        learner.fit(1e-3, 2)
        results = learner.evaluate('val')
    finally:
        Learner.verbose = verbose
    assert len(learner.loss_sched) == 2 * len(data.train_dl) == 6
    assert np.isfinite(learner.loss_sched).all() and np.isfinite(results[0]) and 0.0 <= results[1] <= 1.0
