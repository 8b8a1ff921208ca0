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
"""
import numpy as np
import torch

from . import ops

from .dist import shard_bounds

__all__ = ['DeviceBatches', 'ImageBatches']


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
        imgs = [np.ascontiguousarray(im['img']) for im in ds.images]
        self.shapes = [(a.shape[0], a.shape[1]) for a in imgs]
        desc = np.zeros((self.n, 3), dtype=np.int64)
        desc[:, 1:] = self.shapes
        desc[1:, 0] = np.cumsum([a.size for a in imgs], dtype=np.int64)[:-1]
        self.arena = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(self.device)
        self.desc = torch.from_numpy(desc).to(self.device)
        if ds.ds_type == 'test':
            y = torch.zeros(self.n, dtype=torch.int64)
        elif ds.target_type == 'single_label':
            y = torch.as_tensor(np.asarray(ds.y, dtype=np.int64))
        else:
            y = torch.as_tensor(np.asarray(ds.y, dtype=np.float32))
        self.y = y.to(self.device)

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
