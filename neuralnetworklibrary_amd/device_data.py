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

`ImageStore` is the resident image set itself (K16): built once from decoded arrays or from image FILES (header sizes first, one
arena allocation, threaded Pillow decode chunk by chunk through a pinned staging buffer, optional downscale on upload by
ops.image_resize_u8), with exact channel statistics from ops.image_stats.  Datasets whose images are `ResidentImage` handles of one
store give loaders that read the store's arena: train and validation sets split from one folder share one copy.  A dataset of
decoded arrays goes through `_upload_images` as before.  For handle-backed detection sets the per-image channel means come from
the store's integer table by the same expression as on the array path, float32(sum / (255 H W)) with the quotient in fp64, so the
two agree to the bit (the loaders are tested to within 1 ulp of fp32 of each other, the bound of one rounding).
"""
import numpy as np
import torch

from . import ops

from .dist import shard_bounds

__all__ = ['DeviceBatches', 'ImageBatches', 'DetectionBatches', 'ImageStore', 'ResidentImage', 'decode_image_u8', 'presize_shape']


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


_DEEP_MODES = ('I', 'F', 'I;16', 'I;16B', 'I;16L', 'I;16N')
_RGB_MODES = ('RGB', 'L', 'P', 'RGBA', 'LA', 'CMYK', '1')


def decode_image_u8(path):
    """One image file as a uint8 H x W x 3 RGB array, through Pillow.  No EXIF transpose (cv2.imread(IMREAD_UNCHANGED), which the
    reference's open_image uses, applies none either).  Modes L, P, RGBA, LA, CMYK (and 1) go through .convert('RGB'); 16-bit
    integer and float modes raise ValueError naming the file, as does a file that cannot be decoded.  (Pillow itself reduces a
    16-bit-per-channel RGB PNG to 8 bits on open; such a file arrives as 'RGB' and cannot be told apart here.)"""
    from PIL import Image
    try:
        with Image.open(path) as im:
            if im.mode in _DEEP_MODES:
                raise ValueError('%s: mode %r holds more than 8 bits per channel; convert the file to 8-bit RGB' % (path, im.mode))
            if im.mode not in _RGB_MODES:
                raise ValueError('%s: unsupported image mode %r' % (path, im.mode))
            a = np.asarray(im if im.mode == 'RGB' else im.convert('RGB'), dtype=np.uint8)
    except ValueError:
        raise
    except Exception as e:                                   # Pillow raises OSError / SyntaxError / struct.error on bad files
        raise ValueError('%s: cannot decode the image (%s: %s)' % (path, type(e).__name__, e))
    if a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
        raise ValueError('%s: decoded to shape %r, not H x W x 3' % (path, a.shape))
    return np.ascontiguousarray(a)


def _header_size(path):
    "(H, W) of an image file from its header: nothing is decoded"
    from PIL import Image
    try:
        with Image.open(path) as im:
            w, h = im.size
    except Exception as e:
        raise ValueError('%s: cannot read the image header (%s: %s)' % (path, type(e).__name__, e))
    if h < 1 or w < 1:
        raise ValueError('%s: empty image (%d x %d)' % (path, h, w))
    return int(h), int(w)


def presize_shape(H, W, presize, enlarge=False):
    """The resident (H, W) of an H x W image under `presize`: None keeps it; (h, w) stores every image at that size; an int s stores
    an image whose shorter side exceeds s with the shorter side = s and the longer = int(longer * s / shorter) (save_resized's rule,
    Vision.py:85-88), and a smaller image as it is unless `enlarge`."""
    if presize is None:
        return H, W
    if isinstance(presize, (int, np.integer)):
        s = int(presize)
        if s < 1:
            raise ValueError('presize must be positive (got %r)' % (presize,))
        if min(H, W) <= s and not (enlarge and min(H, W) < s):
            return H, W
        return (s, max(1, int(W * s / H))) if H <= W else (max(1, int(H * s / W)), s)
    h, w = presize
    if int(h) < 1 or int(w) < 1:
        raise ValueError('presize must be positive (got %r)' % (presize,))
    return int(h), int(w)


def _desc_table(shapes):
    "int64 [n, 3] = (byte offset, H, W) of images stored back to back, and the total byte count"
    desc = np.zeros((len(shapes), 3), dtype=np.int64)
    desc[:, 1:] = shapes
    sizes = 3 * desc[:, 1] * desc[:, 2]
    desc[1:, 0] = np.cumsum(sizes)[:-1]
    return desc, int(sizes.sum())


class ResidentImage:
    """Handle of image `index` of an ImageStore: what an ImageDataset carries as images[i]['img'] in place of a decoded array.
    `.shape` is the resident (H, W, 3); `.numpy()` reads the bytes back (tests and displays: it is a device-to-host copy)."""
    __slots__ = ('store', 'index')

    def __init__(self, store, index):
        self.store, self.index = store, int(index)

    @property
    def shape(self):
        H, W = self.store.shapes[self.index]
        return (H, W, 3)

    def numpy(self):
        off, H, W = (int(v) for v in self.store.desc_host[self.index])
        return self.store.arena[off:off + 3 * H * W].cpu().numpy().reshape(H, W, 3)

    def __repr__(self):
        return 'ResidentImage(%d, shape=%r)' % (self.index, self.shape)


class ImageStore:
    """A resident image set, built once and shared by every dataset and loader cut from it: `arena` uint8 [bytes] (HWC RGB images
    back to back) and `desc` int64 [n, 3] (byte offset, H, W) on `device`, the convention of ops.image_aug / ops.detect_aug.
    Attributes: arena, desc, desc_host (numpy copy of desc), shapes [(H, W)] as resident, orig_shapes [(H, W)] as decoded, paths
    (from_files; else None), device.  store[i] is a ResidentImage handle.  Train and validation sets split from one folder hold
    handles of ONE store, so their loaders read one arena."""

    def __init__(self, arena, desc_host, orig_shapes, paths, device):
        self.arena, self.device = arena, device
        self.desc_host = desc_host
        self.desc = torch.from_numpy(desc_host).to(device)
        self.shapes = [(int(h), int(w)) for h, w in desc_host[:, 1:]]
        self.orig_shapes = [(int(h), int(w)) for h, w in orig_shapes]
        self.paths = paths
        self._stats = None

    @staticmethod
    def _device(device):
        from .General.Core import default_device
        return torch.device(device if device is not None else default_device())

    @classmethod
    def from_arrays(cls, arrays, device=None):
        "a store of decoded uint8 H x W x 3 arrays (one host concatenation, one upload)"
        device = cls._device(device)
        imgs = [np.ascontiguousarray(a) for a in arrays]
        for a in imgs:
            if not (a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.size > 0):
                raise ValueError('ImageStore.from_arrays takes non-empty H x W x 3 uint8 arrays')
        if not imgs:
            raise ValueError('ImageStore: no images')
        shapes = [(a.shape[0], a.shape[1]) for a in imgs]
        desc, _ = _desc_table(shapes)
        arena = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(device)
        return cls(arena, desc, shapes, None, device)

    @classmethod
    def from_files(cls, paths, device=None, presize=None, threads=None, chunk_bytes=256 << 20, _enlarge=False):
        """A store of image files.  Every file's size is read from its header first (nothing is decoded), the resident shapes follow
        from `presize` (presize_shape: an int never enlarges) and the arena is allocated ONCE; the files are then decoded
        (decode_image_u8) by `threads` workers, chunk by chunk of at most `chunk_bytes` decoded bytes (a chunk holds at least one
        image), into one pinned staging buffer, and every chunk is copied into its slice of the arena: the host never holds more than
        one chunk decoded.  With `presize` a chunk goes to a temporary device buffer and ops.image_resize_u8 writes its images into
        the arena (needs a CUDA device).  threads: default min(16, NNL_DECODE_THREADS or 8), never above 16, never the CPU count.
        A file whose header cannot be read raises ValueError before anything is allocated; one that fails to decode raises ValueError
        (naming the file) before its chunk is uploaded, and no store is returned."""
        from concurrent.futures import ThreadPoolExecutor
        import os
        device = cls._device(device)
        paths = [str(p) for p in paths]
        if not paths:
            raise ValueError('ImageStore: no images')
        if presize is not None and device.type != 'cuda':
            raise ValueError('ImageStore.from_files: presize resamples on the GPU (ops.image_resize_u8) and needs a CUDA device, got %s' % device)
        if threads is None:
            threads = int(os.environ.get('NNL_DECODE_THREADS', 8))
        threads = max(1, min(16, int(threads)))
        orig = [_header_size(p) for p in paths]
        shapes = [presize_shape(H, W, presize, _enlarge) for H, W in orig]
        desc, total = _desc_table(shapes)
        src_sizes = [3 * H * W for H, W in orig]
        chunks, lo, acc = [], 0, 0                          # [lo, hi) runs of images of at most chunk_bytes decoded bytes
        for i, nb in enumerate(src_sizes):
            if i > lo and acc + nb > chunk_bytes:
                chunks.append((lo, i))
                lo, acc = i, 0
            acc += nb
        chunks.append((lo, len(paths)))
        stage_bytes = max(sum(src_sizes[a:z]) for a, z in chunks)
        arena = torch.empty(total, dtype=torch.uint8, device=device)
        stage = torch.empty(stage_bytes, dtype=torch.uint8, pin_memory=device.type == 'cuda')
        stage_np = stage.numpy()

        def decode(i, off):
            a = decode_image_u8(paths[i])
            if (a.shape[0], a.shape[1]) != orig[i]:
                raise ValueError('%s: decoded to %d x %d, its header says %d x %d' % ((paths[i],) + a.shape[:2] + orig[i]))
            stage_np[off:off + a.size] = a.reshape(-1)

        with ThreadPoolExecutor(max_workers=threads) as pool:
            for a, z in chunks:
                offs = np.concatenate([[0], np.cumsum(src_sizes[a:z])]).astype(np.int64)
                for f in [pool.submit(decode, i, int(offs[i - a])) for i in range(a, z)]:
                    f.result()                               # a ValueError of a worker surfaces here, before the upload
                nb = int(offs[-1])
                if presize is None:
                    d0 = int(desc[a, 0])
                    arena[d0:d0 + nb].copy_(stage[:nb])
                else:
                    tmp = stage[:nb].to(device, non_blocking=True)
                    src = np.stack([offs[:-1], [h for h, _ in orig[a:z]], [w for _, w in orig[a:z]]], axis=1).astype(np.int64)
                    ops.image_resize_u8(tmp, torch.from_numpy(src).to(device), torch.from_numpy(desc[a:z].copy()).to(device), arena)
                if device.type == 'cuda':
                    torch.cuda.current_stream(device).synchronize()     # the staging buffer is written again by the next chunk
        return cls(arena, desc, orig, paths, device)

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, i):
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError('image %d of a store of %d' % (i, len(self)))
        return ResidentImage(self, i % len(self))

    def stats(self, indices=None):
        """uint64 numpy [m, 6]: per image the exact channel sums of v and of v^2 over its resident bytes (ops.image_stats; the whole
        store's table is computed once and kept).  indices: image numbers, default all.  A store that was built on the CPU device
        (no GPU in reach: the listing logic under test) adds the same integers with numpy over its host arena."""
        if self._stats is None and self.device.type == 'cuda':
            self._stats = ops.image_stats(self.arena, self.desc)
        elif self._stats is None:
            flat = self.arena.numpy()
            px = [flat[o:o + 3 * h * w].reshape(-1, 3).astype(np.uint64) for o, h, w in self.desc_host]
            self._stats = np.stack([np.concatenate([p.sum(axis=0, dtype=np.uint64), (p * p).sum(axis=0, dtype=np.uint64)]) for p in px])
        return self._stats.copy() if indices is None else self._stats[np.asarray(indices, dtype=np.int64)]

    def channel_stats(self, indices=None):
        """[means, stds], float64 arrays of 3, with get_stats' definition (Vision.py:93-118): mean_c = the plain average over the
        images of the image's channel mean of v / 255; var_c = the average over the images of the image's channel mean of
        (v / 255)^2, minus mean_c^2 (NOT pixel-weighted).  From the exact integer sums, in fp64: per image one quotient
        sum / (255 H W) resp. sum2 / (255^2 H W), then the average."""
        t = self.stats(indices)
        idx = np.arange(len(self)) if indices is None else np.asarray(indices, dtype=np.int64)
        pixels = np.array([float(self.shapes[i][0] * self.shapes[i][1]) for i in idx], dtype=np.float64)[:, None]
        n = float(len(idx))
        means = (t[:, :3].astype(np.float64) / (255.0 * pixels)).sum(axis=0) / n
        second = (t[:, 3:].astype(np.float64) / (65025.0 * pixels)).sum(axis=0) / n
        return [means, np.sqrt(second - means ** 2)]


def _resident(images, device):
    """The arena of a dataset's images: (host arrays or None, [(H, W)], arena, desc, store or None, image numbers in the store).
    Decoded arrays are concatenated and uploaded (`_upload_images`); ResidentImage handles of ONE store on `device` give the store's
    arena and an index_select of its table: nothing is copied."""
    handles = [isinstance(im['img'], ResidentImage) for im in images]
    if not any(handles):
        return _upload_images(images, device) + (None, None)
    if not all(handles):
        raise ValueError("a dataset's images are either all decoded arrays or all handles of one ImageStore")
    store = images[0]['img'].store
    if any(im['img'].store is not store for im in images):
        raise ValueError("a dataset's image handles must belong to one ImageStore")
    if store.arena.device != torch.empty(0, device=device).device:
        raise ValueError('the ImageStore lives on %s, the loader on %s' % (store.device, device))
    idx = np.array([im['img'].index for im in images], dtype=np.int64)
    desc = store.desc.index_select(0, torch.from_numpy(idx).to(device))
    return None, [store.shapes[i] for i in idx], store.arena, desc, store, idx


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
        _, self.shapes, self.arena, self.desc, self.store, _ = _resident(ds.images, self.device)
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
        imgs, self.shapes, self.arena, self.desc, self.store, store_idx = _resident(ds.images, self.device)
        if self.store is None:
            sums = np.stack([a.reshape(-1, 3).sum(axis=0, dtype=np.int64) for a in imgs])
        else:                                                   # the same exact integers, from the store's device-side table
            sums = self.store.stats(store_idx)[:, :3]
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
