"""Device-resident input pipelines for the array-backed datasets of the reference.

The reference feeds `Learner.fit` through `torch.utils.data.DataLoader` workers: per minibatch a Python `__getitem__` loop,
a numpy collate (`StructuredDataCollater`, StructuredData.py:849-869), a pinned H2D copy and `to_cuda` (Learner.py:599).
For the collaborative-filtering and structured-data heads the whole dataset is a few hundred MB at most (Rossmann:
844 k rows x (32 int64 + 14 fp32) = 263 MB; MovieLens-20M: 20 M x (2 int64 + 1 fp32) = 400 MB) — noise next to 288 GB of HBM
— and a training step takes 0.1-2 ms, so the loader, not the GPU, sets the epoch time.  `DeviceBatches` keeps the arrays in
HBM, draws the epoch permutation on the device and gathers each minibatch there: no workers, no per-step H2D, no host sync.

Data parallelism: every rank holds the full arrays and draws the SAME permutation (seed + epoch), then takes its contiguous
slice of each GLOBAL minibatch — the same partition `dist.ShardedBatches` makes of host batches — so `len()` and the
schedules agree on every rank and the union of the ranks' minibatches is exactly the single-process minibatch.

`ImageBatches` does the same for the vision head's classification datasets (Applications/Vision.py ImageDataset): the decoded
uint8 images live in HBM back to back and each minibatch is cropped, resized, rotate-zoomed, flipped, lit and normalised there
by the HIP augmenter (ops.image_aug) — at 5 520 img/s per GPU the reference's per-image cv2 / numpy Transform.__call__
(Vision.py:449-507) in DataLoader workers, not the training step, would set the epoch time.

`DetectionBatches` is the detection loader (ImageDataset with 'bbox' targets): the same arena, plus every image's boxes and
categories, in HBM; minibatches grouped by aspect ratio (AspectRatioSampler, Vision.py:700-728); one kernel per minibatch
(ops.detect_aug) does TransformBBox.__call__ (:559-603) and AspectRatioCollater (:758-812), whose cv2.resize per image in ONE
DataLoader worker would otherwise set the epoch time of the RetinaNet step.
"""
import numpy as np
import torch

from . import ops

from .dist import shard_bounds

__all__ = ['DeviceBatches', 'ImageBatches', 'DetectionBatches']


def _map(f, x):
    return [_map(f, v) for v in x] if isinstance(x, (list, tuple)) else f(x)


class DeviceBatches:
    """Iterable of (x, y) minibatches gathered on `device` from whole-dataset tensors.

    x: tensor [N, ...] or (nested) list of such tensors (yielded as a list, as the reference's collaters do); y: tensor [N, ...].
    bs: PER-RANK batch size.  shuffle: new permutation every epoch (torch.Generator on the device, seed + epoch).
    rank / world: data-parallel slice of each global minibatch of bs*world samples.  The last minibatch may be ragged
    (the reference's loaders use drop_last=False; Learner scales its learning rate, Learner.py:503-505)."""

    def __init__(self, x, y, bs, shuffle=False, device=None, seed=0, rank=0, world=1):
        from .General.Core import default_device
        self.device = torch.device(device if device is not None else default_device())
        to_dev = lambda t: torch.as_tensor(t).to(self.device)
        self.x, self.y = _map(to_dev, x), to_dev(y)
        self.n = len(self.y)
        self.bs, self.shuffle, self.seed, self.rank, self.world = int(bs), shuffle, int(seed), int(rank), int(world)
        self.epoch = 0
        self._gen = None
        self.dp_info = None          # (rows of the last yielded shard that count, rows of its GLOBAL minibatch): Learner reads it

    def __len__(self):
        g = self.bs * self.world
        return (self.n + g - 1) // g

    def _perm(self):
        if not self.shuffle:
            return None
        if self._gen is None:
            self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self.seed + self.epoch)          # identical on every rank
        return torch.randperm(self.n, device=self.device, generator=self._gen)

    def __iter__(self):
        perm = self._perm()
        self.epoch += 1
        g = self.bs * self.world
        for b in range(len(self)):
            lo = b * g
            hi = min(lo + g, self.n)
            a, z, ghost = shard_bounds(hi - lo, self.rank, self.world)   # balanced contiguous cut, as dist.ShardedBatches
            a, z = lo + a, lo + z
            self.dp_info = (0 if ghost else z - a, hi - lo)
            if perm is None:
                take = lambda t: t[a:z]
            else:
                idx = perm[a:z]
                take = lambda t: t.index_select(0, idx)
            yield _map(take, self.x), take(self.y)


def _upload_images(images, device):
    """The decoded uint8 H x W x 3 arrays of a dataset back to back in one device arena: (host arrays, [(H, W)], arena uint8 [bytes],
    desc int64 [n, 3] = byte offset, H, W per image)"""
    imgs = [np.ascontiguousarray(im['img']) for im in images]
    shapes = [(a.shape[0], a.shape[1]) for a in imgs]
    desc = np.zeros((len(imgs), 3), dtype=np.int64)
    desc[:, 1:] = shapes
    desc[1:, 0] = np.cumsum([a.size for a in imgs], dtype=np.int64)[:-1]
    arena = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(device)
    return imgs, shapes, arena, torch.from_numpy(desc).to(device)


class ImageBatches:
    """Iterable of (x, y) minibatches of an Applications.Vision.ImageDataset, transformed on `device` by ops.image_aug.

    The arena (every image's uint8 HWC bytes back to back), the descriptor table (int64 byte offset, H, W per image) and the
    labels are uploaded once.  Per epoch: a host permutation from np.random.RandomState(seed + epoch) (shuffle=True), and
    from the same stream, per GLOBAL minibatch of bs * world samples and in batch order, one `Transform.sample` draw per
    sample — identical on every rank; a rank then takes its `shard_bounds` slice of the parameter table, uploads it (one small
    H2D per minibatch), launches the kernel(s) on torch's current stream and gathers the labels with index_select.
    Yields x: the logical [n, 3, sz_h, sz_w] view of the kernel's NHWC output (ops.to_nhwc is free), y: int64 [n]
    ('single_label'; zeros for a 'test' dataset) or fp32 [n, ncat] ('multi_label').  The last minibatch may be ragged.
    explicit_params(b, image_indices) -> ops.IMAGE_AUG_PARAM array [len(image_indices)]: replaces the draws for global
    minibatch b (tests inject parameter tables through it)."""

    def __init__(self, ds, bs, shuffle, seed=0, rank=0, world=1, device=None, explicit_params=None):
        from .General.Core import default_device
        self.device = torch.device(device if device is not None else default_device())
        self.ds, self.transform, self.n = ds, ds.transform, len(ds)
        self.bs, self.shuffle, self.seed, self.rank, self.world = int(bs), shuffle, int(seed), int(rank), int(world)
        self.explicit_params = explicit_params
        self.epoch = 0
        self.dp_info = None          # (rows of the last yielded shard that count, rows of its GLOBAL minibatch): Learner reads it
        _, self.shapes, self.arena, self.desc = _upload_images(ds.images, self.device)
        if ds.ds_type == 'test':
            y = torch.zeros(self.n, dtype=torch.int64)
        elif ds.target_type == 'single_label':
            y = torch.as_tensor(np.asarray(ds.y, dtype=np.int64))
        else:
            y = torch.as_tensor(np.asarray(ds.y, dtype=np.float32))
        self.y = y.to(self.device)

    def _view(self, transform, bs, shuffle, seed, rank, world):
        "a loader over THIS loader's arena, descriptor table and labels (nothing is uploaded) with its own transform, batch size and draws"
        v = object.__new__(ImageBatches)
        v.__dict__.update(self.__dict__)
        v.transform, v.bs, v.shuffle, v.seed, v.rank, v.world = transform, int(bs), shuffle, int(seed), int(rank), int(world)
        v.explicit_params, v.epoch, v.dp_info = None, 0, None
        return v

    def with_transform(self, transform, bs=None, shuffle=False, seed=None):
        """A second loader over the SAME device arena, descriptor table and labels — no re-upload — that applies `transform` (an
        Applications.Vision.Transform) with its own batch size (default: this loader's) and seed (default: this loader's).  It is a
        rank-local loader of the full set, as `val_dl` is.  ImageLearner.TTA runs its five transforms over one resident copy of the
        images this way (the reference builds five datasets and DataLoaders, Vision.py:2025-2031)."""
        return self._view(transform, self.bs if bs is None else bs, shuffle, self.seed if seed is None else seed, 0, 1)

    def __len__(self):
        g = self.bs * self.world
        return (self.n + g - 1) // g

    def _table(self, rng, b, idx):
        "the parameter table of GLOBAL minibatch b (image numbers idx): the same rows on every rank"
        if self.explicit_params is not None:
            table = np.ascontiguousarray(self.explicit_params(b, idx), dtype=ops.IMAGE_AUG_PARAM)
            assert table.shape == (len(idx),), 'explicit_params must return one row per sample'
            return table
        shapes = [self.shapes[i] for i in idx]
        return self.transform.param_table(idx, shapes, [self.transform.sample(rng, H, W) for H, W in shapes])

    def __iter__(self):
        rng = np.random.RandomState(self.seed + self.epoch)       # identical on every rank
        perm = rng.permutation(self.n) if self.shuffle else np.arange(self.n)
        self.epoch += 1
        tfm = self.transform
        g = self.bs * self.world
        for b in range(len(self)):
            lo = b * g
            hi = min(lo + g, self.n)
            table = self._table(rng, b, perm[lo:hi])
            a, z, ghost = shard_bounds(hi - lo, self.rank, self.world)   # balanced contiguous cut, as dist.ShardedBatches
            self.dp_info = (0 if ghost else z - a, hi - lo)
            params = torch.from_numpy(table[a:z].view(np.uint8).reshape(z - a, ops.IMAGE_AUG_PARAM.itemsize)).to(self.device)
            out = ops.image_aug(self.arena, self.desc, params, tfm.sz, tfm.stats, lighting=bool(tfm.bal_range))
            idx = params.view(torch.int64)[:, 0]                          # the table's image numbers, already on the device
            yield ops.from_nhwc(out), self.y.index_select(0, idx)


class DetectionBatches:
    """Iterable of (x, [boxes, cats]) minibatches of an Applications.Vision.ImageDataset with 'bbox' targets, built on `device` by
    ops.detect_aug.

    Uploaded once: the image arena and descriptor table (as ImageBatches), every image's channel means of float(v) / 255 (exact
    int64 channel sums taken on the host, divided by 255 H W in float64, rounded to fp32: the mu of the lighting step, Vision.py:576),
    the float64 box arena [total, 4] and the int64 category arena [total]; `box_range` [n, 2] = (first, count) per image.
    grouped=True (train; AspectRatioSampler, :711-728): the image numbers are stably sorted by 'aspect_ratio' and cut into
    consecutive groups of bs * world; every epoch takes the groups in a new order from np.random.RandomState(seed + epoch).
    grouped=False (val, test): groups of bs * world in dataset order.  From the same per-epoch stream, after the group permutation,
    per GLOBAL minibatch and in batch order, one `TransformBBox.sample` per sample — identical on every rank.  rand_scale and the
    jitter of the minibatch are its FIRST sample's (:764-766); resized sizes, Hp, Wp (multiples of 32) and N = max(1, most boxes
    of one image) are those of the global minibatch (TransformBBox.batch_table), so a rank's `shard_bounds` slice of the rows gives
    exactly its rows of the single-process minibatch.  One small H2D per minibatch (the parameter rows), one launch.
    Yields x: the logical [n, 3, Hp, Wp] view of the kernel's NHWC output (ops.to_nhwc is free), [boxes fp32 [n, N, 4], cats int64
    [n, N]] padded with -1 — what SSD_loss and ComputeMaxOverlaps take.  The last group may be ragged.
    explicit_params(b, image_indices) -> [TransformBBox.sample()-style dicts], one per sample: replaces the draws for global
    minibatch b (tests inject draws through it)."""

    def __init__(self, ds, bs, grouped, seed=0, rank=0, world=1, device=None, explicit_params=None):
        from .General.Core import default_device
        self.device = torch.device(device if device is not None else default_device())
        self.ds, self.transform, self.n = ds, ds.transform, len(ds)
        self.bs, self.grouped, self.seed, self.rank, self.world = int(bs), grouped, int(seed), int(rank), int(world)
        self.explicit_params = explicit_params
        self.epoch = 0
        self.dp_info = None          # (rows of the last yielded shard that count, rows of its GLOBAL minibatch): Learner reads it
        self.last_draws = None       # kept by `with_transform` views only
        imgs, self.shapes, self.arena, self.desc = _upload_images(ds.images, self.device)
        sums = np.stack([a.reshape(-1, 3).sum(axis=0, dtype=np.int64) for a in imgs])
        pixels = np.array([255.0 * H * W for H, W in self.shapes], dtype=np.float64)
        self.image_mean = torch.from_numpy((sums.astype(np.float64) / pixels[:, None]).astype(np.float32)).to(self.device)
        self.scales = [float(im['scale']) for im in ds.images]
        boxes, cats, self.box_range = [], [], np.zeros((self.n, 2), dtype=np.int64)
        for i, im in enumerate(ds.images):
            target = 0 if ds.ds_type == 'test' else im['target']                       # ImageDataset.__getitem__, Vision.py:683-686
            if isinstance(target, (int, np.integer)) or len(target) == 0:             # TransformBBox.__call__, :594
                target = []
            self.box_range[i] = (len(boxes), len(target))
            boxes += [np.asarray(b, dtype=np.float64).reshape(4) for b, _ in target]
            cats += [int(c) for _, c in target]
        if not boxes:                                                                  # the arenas are never empty: one unused row
            boxes, cats = [np.zeros(4)], [-1]
        self.box_arena = torch.from_numpy(np.stack(boxes).astype(np.float64)).to(self.device)
        self.cat_arena = torch.from_numpy(np.asarray(cats, dtype=np.int64)).to(self.device)
        g = self.bs * self.world
        if grouped:
            ratios = [im['aspect_ratio'] for im in ds.images]
            order = sorted(range(self.n), key=lambda i: ratios[i])                      # stable, as list.sort (:716)
        else:
            order = list(range(self.n))
        self.groups = [np.array(order[i:i + g], dtype=np.int64) for i in range(0, self.n, g)]

    def with_transform(self, transform, bs=None, seed=None):
        """A second loader over the SAME image arena, descriptor table, channel means, box and category arenas — no re-upload — that
        applies `transform` (an Applications.Vision.TransformBBox) with its own batch size (default: this loader's) and seed (default:
        this loader's): not grouped, dataset order, rank-local over the full set, epoch 0, no explicit_params (as
        ImageBatches.with_transform).  A view REMEMBERS what its last iteration applied: `last_draws[i]` = dict(row_jit, col_jit,
        rand_scale: the values of image i's minibatch, i.e. its first sample's; flip: 1 iff image i was mirrored, the
        NNL_IMAGE_AUG_FLIP flag of its row; rh, rw: its resized size; sample: the TransformBBox.sample() draw of image i itself), None for an image not reached
        yet.  ImageLearner.TTA_bbox runs its five passes over one resident copy of the set this way and undoes them from last_draws
        (the reference builds five datasets and DataLoaders and pre-draws L values per transform copy, Vision.py:2068-2073)."""
        v = object.__new__(DetectionBatches)
        v.__dict__.update(self.__dict__)
        v.transform, v.bs, v.seed = transform, int(self.bs if bs is None else bs), int(self.seed if seed is None else seed)
        v.grouped, v.rank, v.world, v.explicit_params, v.epoch, v.dp_info = False, 0, 1, None, 0, None
        v.groups = [np.arange(i, min(i + v.bs, v.n), dtype=np.int64) for i in range(0, v.n, v.bs)]
        v.last_draws = [None] * v.n
        return v

    def __len__(self):
        return len(self.groups)

    def _table(self, rng, b, idx):
        "the parameter rows and the batch values of GLOBAL minibatch b (image numbers idx): the same on every rank"
        if self.explicit_params is not None:
            draws = list(self.explicit_params(b, idx))
            assert len(draws) == len(idx), 'explicit_params must return one draw per sample'
        else:
            draws = [self.transform.sample(rng) for _ in idx]
        table, v = self.transform.batch_table([int(i) for i in idx], [self.shapes[i] for i in idx], [self.scales[i] for i in idx],
                                              [tuple(self.box_range[i]) for i in idx], draws)
        if self.last_draws is not None:
            for k, i in enumerate(idx):
                self.last_draws[int(i)] = dict(row_jit=v['row_jit'], col_jit=v['col_jit'], rand_scale=v['rand_scale'],
                                               flip=int(bool(table[k]['flags'] & ops.IMAGE_AUG_FLIP)), rh=int(table[k]['rh']),
                                               rw=int(table[k]['rw']), sample=draws[k])
        return table, v

    def __iter__(self):
        rng = np.random.RandomState(self.seed + self.epoch)       # identical on every rank
        order = rng.permutation(len(self.groups)) if self.grouped else np.arange(len(self.groups))
        self.epoch += 1
        tfm = self.transform
        if self.last_draws is not None:
            self.last_draws = [None] * self.n
        for b, gi in enumerate(order):
            idx = self.groups[gi]
            table, v = self._table(rng, b, idx)
            a, z, ghost = shard_bounds(len(idx), self.rank, self.world)   # balanced contiguous cut, as dist.ShardedBatches
            self.dp_info = (0 if ghost else z - a, len(idx))
            params = torch.from_numpy(table[a:z].view(np.uint8).reshape(z - a, ops.DETECT_AUG_PARAM.itemsize)).to(self.device)
            out, boxes, cats = ops.detect_aug(self.arena, self.desc, self.image_mean, self.box_arena, self.cat_arena, params, v['Hp'],
                                              v['Wp'], v['N'], v['row_jit'], v['col_jit'], v['rand_scale'], tfm.stats)
            yield ops.from_nhwc(out), [boxes, cats]
