"""Vision application of the drop-in API: the reference's Applications/Vision.py — data side (§3 Transform / get_transforms
:399-517, §4 ImageDataset / ImageDataObj :642-875 for classification), models and losses (§5 ImageClassificationNet :1203-1373,
§6 ObjectDetectionNet and the SSD loss :1376-1663) and ImageLearner.

On the hot path and HIP-backed: every convolution (ops.conv2d, K1), the classifier head linears, the detection loss —
`SSD_loss.__call__` is ONE fused anchor-match + focal + smooth-L1 kernel per batch (ops.retina_loss, K6) with no host
synchronisation, replacing the reference's per-image Python loop (Vision.py:1636), per-positive-anchor scalar indexing loop (:1593)
and `.nonzero()` syncs (:1506-1507) — and the classification transform chain: the dataset's decoded uint8 images live in HBM and
`device_data.ImageBatches` cuts, crops, resizes, rotate-zooms, flips, lights and normalises each minibatch there (ops.image_aug,
K9), replacing the per-image cv2 / numpy `Transform.__call__` (:449-507) in DataLoader workers.  The detection data side
(TransformBBox :519-612, AspectRatioSampler / AspectRatioCollater :700-812, 'bbox' datasets) works the same way:
`device_data.DetectionBatches` groups the images by aspect ratio and one kernel per minibatch (ops.detect_aug, K10) lights,
normalises, flips, resizes, jitters and pads the images and flips, scales and shifts their boxes in float64.
Image FILES (§1.1 open_image / save_resized / get_stats / get_cat_counts / plot_imgsize_histograms :54-189, §4 ImageDataObj.from_csv /
from_folders / from_json_bbox :901-1200): a folder is decoded once with Pillow into a device_data.ImageStore (threaded, chunked,
optionally downscaled on upload by ops.image_resize_u8, K16), the datasets hold handles of it, and get_stats takes exact integer
channel sums on the device (ops.image_stats, K16).  The data classes also still take decoded H x W x 3 uint8 arrays.
Out of scope here: `pad` and `max_noise` (cv2.GaussianBlur), TransformBBoxShowPreds and TransformBBox.get_values, the display
helpers ShowImages, ShowImages_from_folder and show_image, and ImageLearner's display helpers (show_images, show_bbox_preds)
(SURVEY.md §2.1 rows 9, 12).  Scoring a detector runs on the device too: coco_pascal_eval
(the COCO / Pascal protocol of pycocotools' COCOeval for boxes) and mAP_device (ops.det_eval_coco / ops.det_map, K14).
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..General.Core import *          # noqa: F401,F403
from ..General.Layers import *        # noqa: F401,F403
from ..General.Learner import *       # noqa: F401,F403
from ..General.LossesMetrics import * # noqa: F401,F403
from ..General.Optimizer import *     # noqa: F401,F403
from ..General.Core import TEN, separate_bn_layers
from ..General.Layers import AdaptiveConcatPool2d, Flatten, FullyConnectedNet
from ..General.Learner import Learner
from .VisionModels import vmods
from .VisionModels import resnet as models      # stands in for `torchvision.models` (Vision.py:8)
from .VisionModels.resnet import ResNetBody
from .. import ops

try:  # a torchvision ResNet (if installed) is accepted by default_cut / default_split as well
    import torchvision.models as _tvm
    _RESNET_TYPES = (models.ResNet, _tvm.ResNet)
except Exception:  # torchvision is not installed in this image
    _RESNET_TYPES = (models.ResNet,)

imagenet_stats = [np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])]
alternate_stats = [np.array([0.5, 0.5, 0.5]), np.array([0.5, 0.5, 0.5])]
Pascal_thresholds = [0.5]
COCO_thresholds = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]


# ---- §1.1 general utilities: image files (Vision.py:54-189) --------------------------------------------------------
# ShowImages, ShowImages_from_folder, show_image and TransformBBoxShowPreds (:274-397, :614-640) are display helpers: out of scope.

def _list_images(folder):
    "the entries of `folder`, sorted, without macOS `._*` resource forks (the reference takes os.listdir's arbitrary order)"
    return sorted(f for f in os.listdir(folder) if f[:2] != '._')


def open_image_u8(path):
    """An image file as a uint8 H x W x 3 RGB array (device_data.decode_image_u8): Pillow, no EXIF transpose; L, P, RGBA, LA and CMYK
    files are converted to RGB; 16-bit and float files, and files that cannot be decoded, raise ValueError naming the file."""
    from ..device_data import decode_image_u8
    return decode_image_u8(path)


def open_image(img_name):
    "An image file as float32 RGB in [0, 1], H x W x 3 (Vision.py:54-62), through open_image_u8."
    return open_image_u8(img_name).astype(np.float32) / 255


def _folder_files(img_folder, img_names=None):
    img_folder = correct_foldername(img_folder)
    names = _list_images(img_folder) if img_names is None else list(img_names)
    return img_folder, names


def get_stats(img_folder, img_names=None):
    """[means, stds] (float64 arrays of 3: red, green, blue) over the images `img_names` of `img_folder`, default all of them
    (Vision.py:93-118): the folder is decoded once into a device_data.ImageStore and the moments come from exact integer channel
    sums taken on the GPU (ImageStore.channel_stats; the reference averages float32 per-image means on the host).  mean_c is the
    average over images of the image's channel mean, not pixel-weighted, as in the reference."""
    from ..device_data import ImageStore
    img_folder, names = _folder_files(img_folder, img_names)
    return ImageStore.from_files([img_folder + n for n in names]).channel_stats()


def get_cat_counts(csv_file, skip_first=True, plot_hist=True):
    """Images per category of a single-label csv (`img_name, category` rows; skip_first=False if there is no header row), as a
    DataFrame with columns 'category' and 'count' in descending count; plot_hist also draws the histogram of the counts
    (Vision.py:120-150)."""
    import pandas as pd
    df = pd.read_csv(csv_file, names=['img_name', 'category'], skiprows=1 if skip_first else 0)
    cat_counts = df['category'].value_counts()
    cat_counts = pd.DataFrame({'category': list(cat_counts.index), 'count': list(cat_counts)})
    if plot_hist:
        import matplotlib.pyplot as plt
        plt.hist(cat_counts['count'])
        plt.xlabel('number images in category')
        plt.ylabel('frequency')
    return cat_counts


def plot_imgsize_histograms(foldername, ranges=None, num_bins=10):
    """Histograms of the row sizes, column sizes and aspect ratios (W / H) of the images in `foldername` (Vision.py:152-189).
    ranges = (row_range, col_range, aspect_ratio_range), each [min, max] or None; num_bins: one int or three.  The sizes are read
    from the file headers: nothing is decoded.  Returns (rowsizes, colsizes, aspect_ratios)."""
    import matplotlib.pyplot as plt
    from ..device_data import _header_size
    foldername, names = _folder_files(foldername)
    if ranges is None: ranges = (None, None, None)
    if type(num_bins) == int: num_bins = (num_bins, num_bins, num_bins)
    sizes = [_header_size(foldername + n) for n in names]
    rowsizes, colsizes = [h for h, _ in sizes], [w for _, w in sizes]
    aspect_ratios = [w / h for h, w in sizes]
    plt.figure(figsize=(14, 10))
    for k, (values, title) in enumerate([(rowsizes, 'row sizes'), (colsizes, 'col sizes'), (aspect_ratios, 'aspect ratios')]):
        plt.subplot(2, 2, k + 1)
        plt.hist(values, range=ranges[k], bins=num_bins[k])
        plt.title(title)
    return rowsizes, colsizes, aspect_ratios


def save_resized(img_folder, new_folder, sz):
    """Resized copies of the images of `img_folder` in `new_folder` (Vision.py:64-91).  sz int: the shorter side becomes sz (the longer
    int(longer * sz / shorter)), smaller images are ENLARGED, as in the reference; sz = (h, w): every image becomes h x w.  The folder
    is decoded and resampled on the GPU (ops.image_resize_u8: half-pixel bilinear on float(v), round to nearest even — not the
    fixed-point arithmetic of cv2.resize on uint8, so single bytes may differ by 1 from the reference's files) and Pillow writes the
    files under their own names."""
    from PIL import Image
    from ..device_data import ImageStore
    img_folder, names = _folder_files(img_folder)
    new_folder = correct_foldername(new_folder)
    os.makedirs(new_folder, exist_ok=True)
    for lo in range(0, len(names), 256):                          # a bounded number of images is resident at a time
        part = names[lo:lo + 256]
        store = ImageStore.from_files([img_folder + n for n in part], presize=sz, _enlarge=True)
        for i, n in enumerate(part):
            Image.fromarray(store[i].numpy()).save(new_folder + n)


def jaccard(Boxes1, Boxes2):
    """IoU of every pair (b1, b2): [n,4] x [m,4] -> [n,m], min-max boxes, no +1 (Vision.py:234-256)."""
    if (len(Boxes1) == 0) or (len(Boxes2) == 0):
        return TEN([])
    B1, B2 = Boxes1.float(), Boxes2.float()
    a1 = (B1[:, 2] - B1[:, 0]) * (B1[:, 3] - B1[:, 1])
    a2 = (B2[:, 2] - B2[:, 0]) * (B2[:, 3] - B2[:, 1])
    b1, b2 = B1.unsqueeze(1), B2.unsqueeze(0)
    iw = (torch.min(b1[:, :, 2], b2[:, :, 2]) - torch.max(b1[:, :, 0], b2[:, :, 0])).clamp(min=0)
    ih = (torch.min(b1[:, :, 3], b2[:, :, 3]) - torch.max(b1[:, :, 1], b2[:, :, 1])).clamp(min=0)
    inter = iw * ih
    return inter / (a1.unsqueeze(1) + a2.unsqueeze(0) - inter)


# ---- §1.2 bounding-box utilities (Vision.py:191-269) -------------------------------------------------------------

def hw_to_mm(box):
    "height-width box [xmin, ymin, width, height] -> min-max box [xmin, ymin, xmax, ymax], inclusive pixel ends (Vision.py:191-193)"
    x, y, w, h = box[0], box[1], box[2], box[3]
    return np.array([x, y, x + w - 1, y + h - 1])


def mm_to_hw(box):
    "min-max box [xmin, ymin, xmax, ymax] -> height-width box [xmin, ymin, width, height] (Vision.py:195-197)"
    x0, y0, x1, y1 = box[0], box[1], box[2], box[3]
    return np.array([x0, y0, x1 - x0 + 1, y1 - y0 + 1])


def convert_bbox_list(bbox_list):
    "standard bbox list [(b_1, c_1), ..., (b_n, c_n)] -> (boxes [n, 4], cats [n]) arrays (Vision.py:199-210)"
    return np.array([b for b, _ in bbox_list]), np.array([c for _, c in bbox_list])


def rev_bbox_list(bbox_list):
    """loader form [boxes [N, 4], cats [N]] (tensors or arrays, padded with -1) -> standard bbox list [(b_1, c_1), ..., (b_n, c_n)]:
    everything from the first category -1 on is padding (Vision.py:212-232)"""
    boxes, cats = [ARR(t) if torch.is_tensor(t) else np.asarray(t) for t in bbox_list[:2]]
    out = []
    for b, c in zip(boxes, cats):
        if c == -1:
            break
        out.append((b, c))
    return out


def get_AspectRatioScale(img, min_side, max_side):
    """(aspect_ratio, scale) of an H x W x C image for a 'bbox' dataset (Vision.py:258-269): aspect_ratio = W / H; scale takes the
    shorter side to min_side unless that takes the longer side beyond max_side, then it takes the longer side to max_side."""
    rows, cols = img.shape[0], img.shape[1]
    scale = min_side / min(rows, cols)
    if max(rows, cols) * scale > max_side:
        scale = max_side / max(rows, cols)
    return cols / rows, scale


# ---- §3 image transforms, §4 datasets (classification) -----------------------------------------------------------

_DEVICE_PATH = ('the transform chain runs on the GPU per minibatch: iterate device_data.ImageBatches (ImageDataObj.train_dl / '
                'val_dl / test_dl), which feeds Transform.sample() draws to ops.image_aug')


class Transform(object):
    """Parameters of the classification transform chain (Vision.py:399-507): crop -> resize -> random rotate-zoom -> random
    LR-flip ('SideOn') or dihedral ('TopDown') -> random lighting (balance + contrast) -> normalisation.  Same arguments and
    attributes as the reference.  This class HOLDS the parameters and DRAWS them (`sample`, the reference's draw order); the
    arithmetic is the HIP kernel behind ops.image_aug, run per minibatch by device_data.ImageBatches.
    crop_type: 'center', 'random', a float crop point in [0, 1], or None (the whole image, resized without keeping aspect)."""

    def __init__(self, tfm_type, crop_type, pad=None, sz=224, max_deg=10, max_zoom=1.05,
                 bal_range=[-0.05, 0.05], cont_range=[0.95, 1.05], max_noise=None, stats=imagenet_stats):
        if pad:
            raise NotImplementedError('Transform(pad=...): border padding (cv2.copyMakeBorder) is not part of the device transform chain')
        if max_noise:
            raise NotImplementedError('Transform(max_noise=...): blurred noise (cv2.GaussianBlur) is not part of the device transform chain')
        if sz is None:
            raise NotImplementedError('Transform(sz=None): a minibatch tensor needs one output size; pass sz')
        if tfm_type not in ('Basic', 'SideOn', 'TopDown'):
            raise ValueError("tfm_type must be 'Basic', 'SideOn' or 'TopDown' (got %r)" % (tfm_type,))
        if not (crop_type is None or crop_type in ('center', 'random') or type(crop_type) == float):
            raise ValueError("crop_type must be 'center', 'random', a float or None (got %r)" % (crop_type,))
        if max_deg and not max_zoom:
            raise ValueError('max_deg needs max_zoom: the rotate-zoom step uses both (the reference hits a NameError here)')
        if bal_range and not cont_range:
            raise ValueError('bal_range needs cont_range: the lighting step uses both (the reference hits a NameError here)')
        if type(sz) == int:
            sz = (sz, sz)
        sz = (int(sz[0]), int(sz[1]))
        if tfm_type == 'TopDown' and sz[0] != sz[1]:
            raise ValueError("tfm_type='TopDown' rotates by multiples of 90 degrees and needs a square sz (got %r)" % (sz,))
        self.tfm_type, self.crop_type = tfm_type, crop_type
        self.pad, self.sz, self.max_deg, self.max_zoom = pad, sz, max_deg, max_zoom
        self.bal_range, self.cont_range = bal_range, cont_range
        self.max_noise, self.stats = max_noise, stats

    def __call__(self, img):
        raise NotImplementedError('Transform.__call__ on a host array: ' + _DEVICE_PATH)

    def sample(self, rng, H, W):
        """One image's random parameters from `rng` (np.random.RandomState), drawn in exactly the order of Vision.py:452-481:
        flip, rot, then deg, zoom, bal, cont (each only if its range is set), then the random-crop origin (only for
        crop_type 'random' on a non-square image).  Returns a dict; what was not drawn is None.
        (lo + (hi - lo) * random_sample() IS RandomState.uniform(lo, hi), same stream and same bits, at a sixth of the call cost.)"""
        u = rng.random_sample
        s = dict(flip=int(rng.randint(0, 2)), rot=int(rng.randint(0, 4)), deg=None, zoom=None, bal=None, cont=None, origin=None)
        if self.max_deg: s['deg'] = -self.max_deg + (self.max_deg - -self.max_deg) * u()
        if self.max_zoom: s['zoom'] = 1 + (self.max_zoom - 1) * u()
        if self.bal_range: s['bal'] = self.bal_range[0] + (self.bal_range[1] - self.bal_range[0]) * u()
        if self.cont_range: s['cont'] = self.cont_range[0] + (self.cont_range[1] - self.cont_range[0]) * u()
        if self.crop_type == 'random' and H != W:
            s['origin'] = int(rng.randint(0, abs(H - W) + 1))
        return s

    def crop_windows(self, H, W, origin=None):
        """(y, x, h, w) arrays of the crops of images H x W (int arrays) (Vision.py:469-481); origin: the drawn offsets along the
        longer side for crop_type 'random'"""
        H, W = np.asarray(H, dtype=np.int64), np.asarray(W, dtype=np.int64)
        zero = np.zeros_like(H)
        if self.crop_type is None:
            return zero, zero, H, W
        L = np.minimum(H, W)
        slack = np.maximum(H, W) - L
        if self.crop_type == 'center': o = slack // 2
        elif self.crop_type == 'random': o = np.where(slack > 0, np.asarray(origin, dtype=np.int64), 0)
        else: o = (slack * self.crop_type).astype(np.int64)                      # int((rows - L) * crop_point)
        return np.where(H > L, o, 0), np.where(H > L, 0, o), L, L

    def inverse_maps(self, deg, zoom):
        """[n, 6] coefficients that take a pixel of cv2.warpAffine's output back to its source coordinate: the inverses of
        cv2.getRotationMatrix2D((sz_w // 2, sz_h // 2), deg, zoom) (Vision.py:488), computed in float64 and rounded to fp32."""
        deg, zoom = np.asarray(deg, dtype=np.float64), np.asarray(zoom, dtype=np.float64)
        a, b = zoom * np.cos(np.radians(deg)), zoom * np.sin(np.radians(deg))
        cx, cy = self.sz[1] // 2, self.sz[0] // 2
        M = np.zeros((len(deg), 3, 3), dtype=np.float64)
        M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = a, b, (1 - a) * cx - b * cy
        M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = -b, a, b * cx + (1 - a) * cy
        M[:, 2, 2] = 1
        return np.linalg.inv(M)[:, :2].reshape(-1, 6).astype(np.float32)

    def param_table(self, images, shapes, draws):
        """ops.IMAGE_AUG_PARAM rows for image numbers `images` of sizes `shapes` [(H, W)] from `draws` [sample() dicts, or chosen
        values].  As in the reference, flip counts for 'SideOn' / 'TopDown' only and rot for 'TopDown' only (:492-493); the
        rotate-zoom runs iff max_deg is set (:487) and the lighting iff bal_range is (:496)."""
        n = len(images)
        t = np.zeros(n, dtype=ops.IMAGE_AUG_PARAM)
        col = lambda k, dtype: np.array([d[k] for d in draws], dtype=dtype)
        hw = np.asarray(shapes, dtype=np.int64).reshape(n, 2)
        t['image'] = images
        t['crop_y'], t['crop_x'], t['crop_h'], t['crop_w'] = self.crop_windows(
            hw[:, 0], hw[:, 1], [d.get('origin') or 0 for d in draws] if self.crop_type == 'random' else None)
        flags = np.zeros(n, dtype=np.int32)
        if self.max_deg: t['m'] = self.inverse_maps(col('deg', np.float64), col('zoom', np.float64))
        else: flags |= ops.IMAGE_AUG_NO_WARP
        if self.tfm_type in ('SideOn', 'TopDown'): flags |= np.where(col('flip', np.int32) == 1, ops.IMAGE_AUG_FLIP, 0).astype(np.int32)
        if self.tfm_type == 'TopDown': t['rot'] = col('rot', np.int32)
        if self.bal_range: t['bal'], t['cont'] = col('bal', np.float64), col('cont', np.float64)
        else: flags |= ops.IMAGE_AUG_NO_LIGHTING
        t['flags'] = flags
        return t

    def param_row(self, image, H, W, flip=0, rot=0, deg=None, zoom=None, bal=None, cont=None, origin=None):
        "param_table for one image: a 0-d ops.IMAGE_AUG_PARAM record"
        return self.param_table([image], [(H, W)], [dict(flip=flip, rot=rot, deg=deg, zoom=zoom, bal=bal, cont=cont, origin=origin)])[0]


def get_transforms(tfm_type, sz=224, stats=imagenet_stats):
    """[tfm_eval, tfm_aug] for single_label / multi_label classification (Vision.py:509-517): tfm_aug trains, tfm_eval serves
    val and test."""
    tfm_eval = Transform('Basic', 'center', None, sz, None, None, None, None, stats=stats)
    tfm_aug = Transform(tfm_type, 'random', None, sz, stats=stats)
    return [tfm_eval, tfm_aug]


_DEVICE_PATH_BBOX = ('the detection transform and collater run on the GPU per minibatch: iterate device_data.DetectionBatches '
                     "(ImageDataObj(..., 'bbox', ...).train_dl / val_dl / test_dl), which feeds TransformBBox.sample() draws to ops.detect_aug")


class TransformBBox(object):
    """Parameters of the detection transform (Vision.py:519-603): random lighting (balance + contrast about the image's channel
    means) -> normalisation -> random LR-flip ('SideOn') of image and boxes; rand_scale and the jitter are drawn per image and
    applied per minibatch by the collater (:758-812), which resizes every image by scale * rand_scale, pads it on the top and left
    by the jitter and pads the minibatch to a multiple of 32.  Same arguments and attributes as the reference.  This class HOLDS
    the parameters and DRAWS them (`sample`, the reference's draw order); the arithmetic is the HIP kernel behind ops.detect_aug,
    run per minibatch by device_data.DetectionBatches.  L (the length of the reference's pre-drawn value lists) is kept and unused."""

    def __init__(self, tfm_type, bal_range=[-0.05, 0.05], cont_range=[0.95, 1.05], stats=imagenet_stats, scale_range=[0.8, 1.2],
                 jitter=20, L=100000):
        if tfm_type not in ('Basic', 'SideOn'):
            raise ValueError("tfm_type must be 'Basic' or 'SideOn' (got %r)" % (tfm_type,))
        if bal_range and not cont_range:
            raise ValueError('bal_range needs cont_range: the lighting step uses both (the reference hits a TypeError here)')
        if int(jitter) < 0:
            raise ValueError('jitter must be >= 0 (got %r)' % (jitter,))
        self.tfm_type, self.stats, self.jitter, self.L = tfm_type, stats, jitter, L
        self.scale_range, self.bal_range, self.cont_range = scale_range, bal_range, cont_range
        self.iter = None

    def get_values(self):
        raise NotImplementedError('TransformBBox.get_values (pre-drawn values for TTA_bbox) is not built: ' + _DEVICE_PATH_BBOX)

    def __call__(self, img, target):
        raise NotImplementedError('TransformBBox.__call__ on a host array: ' + _DEVICE_PATH_BBOX)

    def sample(self, rng):
        """One image's random parameters from `rng` (np.random.RandomState), drawn in exactly the order of Vision.py:565-575:
        row_jit, col_jit, flip (drawn for 'Basic' too), rand_scale, then bal and cont (only if bal_range is set; else None)."""
        s = dict(row_jit=int(rng.randint(0, self.jitter + 1)), col_jit=int(rng.randint(0, self.jitter + 1)),
                 flip=int(rng.randint(0, 2)), rand_scale=float(rng.uniform(self.scale_range[0], self.scale_range[1])),
                 bal=None, cont=None)
        if self.bal_range:
            s['bal'] = float(rng.uniform(self.bal_range[0], self.bal_range[1]))
            s['cont'] = float(rng.uniform(self.cont_range[0], self.cont_range[1]))
        return s

    def batch_table(self, images, shapes, scales, box_ranges, draws):
        """What the collater makes of one minibatch (Vision.py:764-766, 774, 790-792, 799): image numbers `images` of sizes `shapes`
        [(H, W)], intrinsic `scales`, `box_ranges` [(first, count)] in the box arena and `draws` [sample() dicts, or chosen values]
        -> (ops.DETECT_AUG_PARAM rows, dict(rand_scale, row_jit, col_jit, Hp, Wp, N)).  rand_scale and the jitter are those of the
        FIRST sample; flip counts for 'SideOn' only (:583, :598) and the lighting runs iff bal_range is set (:573)."""
        n = len(images)
        rand_scale, row_jit, col_jit = float(draws[0]['rand_scale']), int(draws[0]['row_jit']), int(draws[0]['col_jit'])
        t = np.zeros(n, dtype=ops.DETECT_AUG_PARAM)
        for k in range(n):
            (H, W), scale = shapes[k], float(scales[k])
            rw, rh = int(W * scale * rand_scale), int(H * scale * rand_scale)                   # cv2.resize(img, (rw, rh)), :774
            if rw < 1 or rh < 1:
                raise ValueError('image %d (%d x %d) resized by scale %r * rand_scale %r has an empty side (%d x %d)'
                                 % (images[k], H, W, scale, rand_scale, rh, rw))
            flags = 0
            if self.tfm_type == 'SideOn' and draws[k]['flip'] == 1: flags |= ops.IMAGE_AUG_FLIP
            if self.bal_range: t[k]['bal'], t[k]['cont'] = draws[k]['bal'], draws[k]['cont']
            else: flags |= ops.IMAGE_AUG_NO_LIGHTING
            t[k]['image'], t[k]['rh'], t[k]['rw'], t[k]['flags'], t[k]['scale'] = images[k], rh, rw, flags, scale
            t[k]['box_first'], t[k]['box_count'] = box_ranges[k]
        Hp = 32 * -(-int(t['rh'].max() + row_jit) // 32)
        Wp = 32 * -(-int(t['rw'].max() + col_jit) // 32)
        return t, dict(rand_scale=rand_scale, row_jit=row_jit, col_jit=col_jit, Hp=Hp, Wp=Wp, N=max(1, int(t['box_count'].max())))


def get_transforms_bbox(tfm_type, jitter=20, scale_range=[0.8, 1.2]):
    """[tfm_eval, tfm_aug] for bounding-box object detection (Vision.py:605-612): tfm_aug trains, tfm_eval (no lighting, no flip, no
    jitter, rand_scale 1) serves val and test."""
    tfm_eval = TransformBBox('Basic', None, None, jitter=0, scale_range=[1, 1])
    tfm_aug = TransformBBox(tfm_type, jitter=jitter, scale_range=scale_range)
    return [tfm_eval, tfm_aug]


class ImageDataset(object):
    """Image dataset for single_label / multi_label classification or bbox object detection (Vision.py:642-698), 'train', 'val' or
    'test'.  images: list of {'img': H x W x 3 uint8 array (decoded RGB), 'target': int label | 0-1 array | 0 for test}; for 'bbox'
    'target' is a standard bbox list [(box [xmin, ymin, xmax, ymax], category), ...] (or [] or 0) and every image also carries
    'scale' and 'aspect_ratio' (get_AspectRatioScale), as the reference's from_json_bbox stores them.  The reference keeps file
    names under 'img' and decodes per item; here 'img' is a decoded array or a device_data.ResidentImage (a handle of an image that
    an ImageStore already decoded and uploaded: what from_csv / from_folders / from_json_bbox put there, next to 'file', the name
    relative to IMG_PATH), and a file name raises.
    Attributes as the reference: IMG_PATH, images, transform, target_type, ds_type, y."""

    def __init__(self, IMG_PATH, images, transform, target_type, ds_type):
        if target_type == 'bbox' and not isinstance(transform, TransformBBox):
            raise NotImplementedError("target_type 'bbox' needs a TransformBBox (get_transforms_bbox): the classification Transform crops "
                                      "and resizes to one size and does not move bbox targets")
        if target_type != 'bbox' and isinstance(transform, TransformBBox):
            raise ValueError("a TransformBBox goes with target_type 'bbox' (got %r): classification datasets take a Transform (get_transforms)" % (target_type,))
        if target_type not in ('single_label', 'multi_label', 'bbox'):
            raise ValueError("target_type must be 'single_label', 'multi_label' or 'bbox' (got %r)" % (target_type,))
        if target_type == 'bbox':
            for im in images:
                if 'scale' not in im or 'aspect_ratio' not in im:
                    raise ValueError("a 'bbox' dataset needs images[i]['scale'] and images[i]['aspect_ratio']: "
                                     "aspect_ratio, scale = get_AspectRatioScale(img, min_side, max_side)")
        from ..device_data import ResidentImage
        for im in images:
            a = im['img']
            if isinstance(a, str):
                raise NotImplementedError("images[i]['img'] is a file name: an ImageDataset does not decode per item; build the data with "
                                          "ImageDataObj.from_csv / from_folders / from_json_bbox (or device_data.ImageStore.from_files), or "
                                          "pass the decoded H x W x 3 uint8 array")
            if isinstance(a, ResidentImage):
                continue
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.size > 0):
                raise ValueError("images[i]['img'] must be a non-empty H x W x 3 uint8 array or a device_data.ResidentImage")
        self.IMG_PATH = IMG_PATH
        self.images = images
        self.transform = transform
        self.target_type = target_type
        self.ds_type = ds_type
        self.y = [images[i]['target'] for i in range(len(images))]

    def __len__(self):
        return len(self.images)

    def __getitem__(self, idx):
        raise NotImplementedError('ImageDataset[i] would transform one image on the host: ' + _DEVICE_PATH)


class ImageDataObj(object):
    """Datasets and loaders for train, validation and (optionally) test data (Vision.py:814-875), classification targets.
    transforms = [tfm_eval, tfm_aug]: tfm_aug trains, tfm_eval serves val and test.  Attributes as the reference: categories,
    target_type, bs, sz, train_ds / val_ds / test_ds, train_dl / val_dl / test_dl (test_* are None unless test_name is given).
    The loaders are device_data.ImageBatches: the images are uploaded once and every minibatch is cut and transformed on the
    GPU, so `num_workers` is accepted and ignored; `seed` seeds the epoch permutations and the transform draws.
    target_type 'bbox' (transforms = get_transforms_bbox(...)): the loaders are device_data.DetectionBatches; train_dl groups the
    images by aspect ratio into minibatches of bs (AspectRatioSampler, :700-728), val_dl and test_dl have batch size 1 in dataset
    order (:865-870; Learner.predict relies on it), and sz is None: every minibatch has its own padded size.
    The file-based constructors from_csv, from_folders and from_json_bbox (Vision.py:901-1200) decode every image folder once into
    a device_data.ImageStore and hand the datasets handles of it: train and validation sets split from one folder share one arena."""

    def __init__(self, PATH, target_type, categories, bs, transforms, train_images, val_images,
                 test_images=None, train_name='train', val_name='val', test_name=None, num_workers=8, seed=0):
        from ..device_data import DetectionBatches, ImageBatches
        tfm_eval, tfm_aug = transforms[0], transforms[1]
        self.target_type, self.categories, self.bs = target_type, categories, bs
        self.sz = tfm_eval.sz if target_type != 'bbox' else None

        PATH = correct_foldername(PATH)
        self.train_ds = ImageDataset(PATH + train_name + '/', train_images, tfm_aug, target_type, 'train')
        self.val_ds = ImageDataset(PATH + val_name + '/', val_images, tfm_eval, target_type, 'val')
        if test_name: self.test_ds = ImageDataset(PATH + test_name + '/', test_images, tfm_eval, target_type, 'test')
        else: self.test_ds = None

        from .. import dist as nnl_dist                    # under torch.distributed every rank takes its slice of each global minibatch
        if target_type == 'bbox':
            self.train_dl = DetectionBatches(self.train_ds, bs, grouped=True, seed=seed, rank=nnl_dist.rank(), world=nnl_dist.world_size())
            self.val_dl = DetectionBatches(self.val_ds, 1, grouped=False, seed=seed)
            self.test_dl = DetectionBatches(self.test_ds, 1, grouped=False, seed=seed) if test_name else None
            return
        self.train_dl = ImageBatches(self.train_ds, bs, shuffle=True, seed=seed, rank=nnl_dist.rank(), world=nnl_dist.world_size())
        self.val_dl = ImageBatches(self.val_ds, bs, shuffle=False, seed=seed)
        if test_name: self.test_dl = ImageBatches(self.test_ds, bs, shuffle=False, seed=seed)
        else: self.test_dl = None

    def get_stats(self, ds_type='train'):
        """[means, stds] of the 'train', 'val' or 'test' set as the module-level get_stats defines them, from the images that are
        already resident: nothing is decoded again (a set of decoded arrays is uploaded to a store of its own for the call)."""
        from ..device_data import ImageStore, ResidentImage
        ds = getattr(self, ds_type + '_ds')
        if ds is None:
            raise ValueError('this ImageDataObj has no %r set' % (ds_type,))
        imgs = [im['img'] for im in ds.images]
        if isinstance(imgs[0], ResidentImage):
            return imgs[0].store.channel_stats([h.index for h in imgs])
        return ImageStore.from_arrays(imgs).channel_stats()

    @staticmethod
    def convert_labels_multi(targets, categories_rev):
        """[category names] per image -> float32 presence / absence vectors over `categories_rev` (name -> index), Vision.py:876-898
        (which rewrites a DataFrame column in place; this takes and returns lists).  An unknown category raises ValueError naming it."""
        out = []
        for names in targets:
            v = np.zeros(len(categories_rev))
            for name in names:
                if name not in categories_rev:
                    raise ValueError('category %r is not among the categories of the training csv' % (name,))
                v[categories_rev[name]] = 1
            out.append(v.astype('float32'))
        return out

    @staticmethod
    def _stores(PATH, folder_files, presize, decode_threads):
        "{folder: {file name: ResidentImage}}: ONE ImageStore per image folder, over the files that are asked of it in first-seen order"
        from ..device_data import ImageStore
        handles = {}
        for folder, files in folder_files.items():
            names = list(dict.fromkeys(files))
            store = ImageStore.from_files([PATH + folder + '/' + f for f in names], presize=presize, threads=decode_threads)
            handles[folder] = {f: store[i] for i, f in enumerate(names)}
        return handles

    @classmethod
    def from_csv(cls, PATH, transforms, bs, train_csv='train.csv', val_csv=None, test_csv=None, train_name='train',
                 val_name=None, test_name=None, target_type='single_label', val_frac=0.2, skip_first=True, suffix='',
                 *, presize=None, seed=0, decode_threads=None):
        """An ImageDataObj from csv files, 'single_label' or 'multi_label' (Vision.py:901-1014; same arguments, order and defaults).
        PATH holds the image folders train_name / val_name / test_name and the csv files train_csv / val_csv / test_csv, rows
        `img, category` (single) or `img, cat1 cat2 ...` (multi), with a header row iff skip_first.  suffix is appended to every
        csv file name.  Without val_name a random val_frac of the training rows becomes the validation set (SplitTrainVal, which
        draws from numpy's GLOBAL generator as the reference does: np.random.seed(k) fixes the split) and both sets read ONE
        resident copy of the training folder.  A test folder needs no csv: its files are listed.  categories: the sorted category
        names of the TRAINING csv; targets: int64 labels, or float32 presence vectors.
        Keyword-only additions: presize (device_data.ImageStore.from_files: store large images downscaled, never enlarged), seed (of
        the loaders' permutations and transform draws), decode_threads.
        Deliberate differences from the reference: a listed test folder is sorted and its `._*` files are skipped (os.listdir order
        is arbitrary); a category of a val / test csv that the training csv lacks raises ValueError naming it (the reference fails
        later, in a cast); nothing is printed; every image is decoded HERE, once, so an unreadable file raises at construction."""
        import pandas as pd
        if target_type not in ('single_label', 'multi_label'):
            raise ValueError("from_csv builds 'single_label' or 'multi_label' data (got %r)" % (target_type,))
        PATH = correct_foldername(PATH)

        def read(csv_name):
            df = pd.read_csv(PATH + csv_name, names=['img_name', 'target'], skiprows=1 if skip_first else 0)
            target = df['target'].str.split() if target_type == 'multi_label' else df['target']
            return [{'img_name': n, 'target': t} for n, t in zip(df['img_name'], target)]

        TRAIN = read(train_csv)
        if target_type == 'single_label':
            category_names = sorted(set(r['target'] for r in TRAIN))
        else:
            category_names = sorted(set(cat for r in TRAIN for cat in r['target']))
        categories = {i: category_names[i] for i in range(len(category_names))}
        categories_rev = {category_names[i]: i for i in range(len(category_names))}

        if val_csv:
            VAL = read(val_csv)
        else:
            TRAIN, VAL = SplitTrainVal(TRAIN, val_frac=val_frac)
            val_name = train_name
        if test_name and test_csv:
            TEST = read(test_csv)
        elif test_name:
            TEST = [{'img_name': f, 'target': 0} for f in _list_images(PATH + test_name)]
        else:
            TEST = None

        def convert(rows, labelled, add_suffix):
            names = [str(r['img_name']) + (suffix if add_suffix else '') for r in rows]
            if not labelled:
                return names, [r['target'] for r in rows]
            if target_type == 'multi_label':
                return names, cls.convert_labels_multi([r['target'] for r in rows], categories_rev)
            for r in rows:
                if r['target'] not in categories_rev:
                    raise ValueError('category %r is not among the categories of the training csv' % (r['target'],))
            return names, [int(categories_rev[r['target']]) for r in rows]

        sets = {'train': (train_name,) + convert(TRAIN, True, True), 'val': (val_name,) + convert(VAL, True, True)}
        if TEST is not None:
            sets['test'] = (test_name,) + convert(TEST, bool(test_csv), bool(test_csv))
        return cls._from_lists(PATH, target_type, categories, bs, transforms, sets, train_name, val_name, test_name, presize, seed,
                               decode_threads)

    @classmethod
    def _from_lists(cls, PATH, target_type, categories, bs, transforms, sets, train_name, val_name, test_name, presize, seed,
                    decode_threads, extra=None):
        """sets: {'train' | 'val' | 'test': (folder, [file names], [targets])} -> the stores (one per folder), the image lists with
        handles, then cls(...).  extra: {'train' | ...: [dict of further keys per image]} ('bbox': id, aspect_ratio, scale)."""
        folder_files = {}
        for folder, names, _ in sets.values():
            folder_files.setdefault(folder, []).extend(names)
        handles = cls._stores(PATH, folder_files, presize, decode_threads)
        lists = {}
        for k, (folder, names, targets) in sets.items():
            lists[k] = [dict({'img': handles[folder][f], 'file': f, 'target': t}, **(extra[k][i] if extra else {}))
                        for i, (f, t) in enumerate(zip(names, targets))]
        return cls(PATH, target_type, categories, bs, transforms, lists['train'], lists['val'], lists.get('test'),
                   train_name, val_name, test_name, seed=seed)

    @classmethod
    def from_folders(cls, PATH, transforms, bs, train_name='train', val_name=None, test_name=None, val_frac=0.2,
                     *, presize=None, seed=0, decode_threads=None):
        """A 'single_label' ImageDataObj from labelled folders (Vision.py:1016-1060; same arguments, order and defaults):
        PATH/train_name (and PATH/val_name) hold one sub-folder per category with that category's images; PATH/test_name holds the
        test images themselves.  Without val_name a random val_frac of the training images becomes the validation set (SplitTrainVal:
        numpy's global generator) and both sets read one resident copy.  Image names are 'category/file'.
        Keyword-only additions: presize, seed, decode_threads (see from_csv).  Deliberate differences: every os.listdir result is
        sorted and `._*` entries are skipped (categories and files); nothing is printed."""
        PATH = correct_foldername(PATH)
        category_names = _list_images(PATH + train_name)
        categories = {i: category_names[i] for i in range(len(category_names))}
        categories_rev = {category_names[i]: i for i in range(len(category_names))}

        def labelled(folder):
            return [{'img': cat + '/' + f, 'target': categories_rev[cat]} for cat in category_names for f in _list_images(PATH + folder + '/' + cat)]

        train_images = labelled(train_name)
        if val_name:
            val_images = labelled(val_name)
        else:
            val_name = train_name
            train_images, val_images = SplitTrainVal(train_images, val_frac=val_frac)
        rows = lambda folder, L: (folder, [r['img'] for r in L], [r['target'] for r in L])
        sets = {'train': rows(train_name, train_images), 'val': rows(val_name, val_images)}
        if test_name:
            test_files = _list_images(PATH + test_name)
            sets['test'] = (test_name, test_files, [0] * len(test_files))
        return cls._from_lists(PATH, 'single_label', categories, bs, transforms, sets, train_name, val_name, test_name, presize, seed,
                               decode_threads)

    @classmethod
    def from_json_bbox(cls, PATH, transforms, bs, train_json='train.json', val_json=None, test_json=None,
                       train_name='train', val_name=None, test_name=None, val_frac=0.2, suffix='', get_ARS=[608, 1216],
                       *, presize=None, seed=0, decode_threads=None):
        """A 'bbox' ImageDataObj from COCO / Pascal style json annotation files (Vision.py:1062-1200; same arguments, order and
        defaults).  A json holds 'categories' [{id, name}], 'images' [{id, file_name}] and 'annotations' [{image_id, bbox = [xmin,
        ymin, width, height], category_id}].  categories: index -> name in the TRAINING json's order; data.cat2dscat: index -> dataset
        category id.  Annotations with ignore == 1 or iscrowd == 1 are skipped; boxes become min-max boxes (hw_to_mm); every image
        carries 'id', 'aspect_ratio' and 'scale' = get_AspectRatioScale(size, *get_ARS), the size read from the file's HEADER (the
        reference decodes every image for it).  Without val_name a random val_frac of the training images is the validation set
        (SplitTrainVal: numpy's global generator), sharing the resident copy.  val_dl and test_dl have batch size 1.
        Keyword-only additions: seed, decode_threads (see from_csv); presize is refused with ValueError: boxes and 'scale' are in
        original pixels.  Deliberate differences: a listed test folder is sorted (its `._*` files are skipped, as in the reference);
        nothing is printed."""
        import json
        if presize is not None:
            raise ValueError("from_json_bbox stores the images at their original size: boxes and 'scale' are in original pixels (presize=%r)" % (presize,))
        from ..device_data import _header_size
        PATH = correct_foldername(PATH)

        def load(name):
            with open(PATH + name) as f:
                return json.load(f)

        trn_json = load(train_json)
        val_json = load(val_json) if val_json else None
        test_json = load(test_json) if test_json else None
        cats = trn_json['categories']
        categories = {i: cats[i]['name'] for i in range(len(cats))}
        cat2dscat = {i: cats[i]['id'] for i in range(len(cats))}
        dscat2cat = {v: k for k, v in cat2dscat.items()}

        def ars(folder, img_name):
            H, W = _header_size(PATH + folder + '/' + img_name)
            return get_AspectRatioScale(np.broadcast_to(np.uint8(0), (H, W, 3)), get_ARS[0], get_ARS[1])

        def annotated(js, folder):
            images = {}
            for image in js['images']:
                ID, img_name = image['id'], image['file_name'] + suffix
                images[ID] = {'id': ID, 'img': img_name, 'target': []}
                if folder is not None:
                    images[ID]['aspect_ratio'], images[ID]['scale'] = ars(folder, img_name)
            for ann in js['annotations']:
                if (('ignore' in ann) and (ann['ignore'] == 1)) or (('iscrowd' in ann) and (ann['iscrowd'] == 1)):
                    continue
                images[ann['image_id']]['target'].append((hw_to_mm(ann['bbox']), dscat2cat[ann['category_id']]))
            return list(images.values())

        train_images = annotated(trn_json, train_name)
        if val_name:
            val_images = annotated(val_json, val_name)
        else:
            train_images, val_images = SplitTrainVal(train_images, val_frac=val_frac)
            val_name = train_name
        if test_name and test_json:
            test_images = annotated(test_json, None)
        elif test_name:
            test_images = [{'img': fn, 'target': 0} for fn in _list_images(PATH + test_name)]
        else:
            test_images = None
        if test_name:
            for im in test_images:
                im['aspect_ratio'], im['scale'] = ars(test_name, im['img'])

        def rows(folder, L):
            return (folder, [r['img'] for r in L], [r['target'] for r in L])
        keys = lambda L: [{k: v for k, v in r.items() if k not in ('img', 'target')} for r in L]
        sets = {'train': rows(train_name, train_images), 'val': rows(val_name, val_images)}
        extra = {'train': keys(train_images), 'val': keys(val_images)}
        if test_name:
            sets['test'], extra['test'] = rows(test_name, test_images), keys(test_images)
        data = cls._from_lists(PATH, 'bbox', categories, bs, transforms, sets, train_name, val_name, test_name, None, seed,
                               decode_threads, extra)
        data.cat2dscat = cat2dscat
        return data


# ---- §5 image classification ---------------------------------------------------------------------------------

def default_cut(model):
    """Cut a known body arch before its pooling / classifier (Vision.py:1205-1219)."""
    if isinstance(model, _RESNET_TYPES):
        return ResNetBody(*list(model.children())[:-2])
    if isinstance(model, (vmods.ResNeXt101_32x4d, vmods.ResNeXt101_64x4d, vmods.InceptionV4)):
        return model.features
    if isinstance(model, vmods.SENet):
        return nn.Sequential(*list(model.children())[:5])
    return model


def default_split(precut_body, body):
    """Split a known body arch into 2 layer groups about half way (Vision.py:1221-1242)."""
    kids = list(body.children())
    if isinstance(precut_body, _RESNET_TYPES) or isinstance(precut_body, (vmods.ResNeXt101_32x4d, vmods.ResNeXt101_64x4d)):
        return [nn.Sequential(*kids[:6]), nn.Sequential(*kids[6:])]
    if isinstance(precut_body, vmods.SENet):
        return [nn.Sequential(*kids[:3]), nn.Sequential(*kids[3:])]
    if isinstance(precut_body, vmods.InceptionV4):
        return [nn.Sequential(*kids[:11]), nn.Sequential(*kids[11:])]
    return [body]


def _num_features(body, data):
    """Channel count of the body's output.  The reference pushes a zero image through the training-mode body
    (Vision.py:1312-1313), which as a side effect moves every BN running stat one momentum step towards (0, 0); with a
    GPU present the same probe runs here (on the device: the HIP body has no CPU path) so the buffers match.  Without
    a GPU (host-logic tests) the count is the body's own `num_features` (a body whose output is a concatenation, NASNetALarge), or
    is read off the last conv / batch-norm."""
    if torch.cuda.is_available():
        dev = default_device()
        with torch.no_grad():
            return body.to(dev)(torch.zeros(1, 3, data.sz[0], data.sz[1], device=dev)).shape[1]
    last = getattr(body, 'num_features', None)
    if isinstance(last, int):
        return last
    last = None
    for m in body.modules():
        if isinstance(m, nn.BatchNorm2d):
            last = m.num_features
        elif isinstance(m, nn.Conv2d):
            last = m.out_channels
    if last is not None:
        return last
    dev = default_device()
    with torch.no_grad():
        return body.to(dev)(torch.zeros(1, 3, data.sz[0], data.sz[1], device=dev)).shape[1]


class ImageClassificationNet(nn.Module):
    """Pretrained-style `body` + `head` classifier (Vision.py:1244-1337).  head default:
    AdaptiveConcatPool2d -> Flatten -> FullyConnectedNet([2*nfeats, 512, ncats], drops [.25,.25]);
    layer_groups = body groups (default_split) + [head]."""

    def __init__(self, data, arch, head='default', cutpoint='default', splits='default'):
        super().__init__()
        if cutpoint is None:
            self.body = arch
        elif cutpoint == 'default':
            self.body = default_cut(arch)
        elif type(cutpoint) == int:
            self.body = nn.Sequential(*list(arch.children())[:cutpoint])

        if isinstance(head, nn.Module):
            self.head = head
        else:
            if type(head) == list:
                layer_sizes, drops = head[0], head[1]
            elif head == 'default':
                layer_sizes, drops = [512], [0.25, 0.25]
            nfeats = _num_features(self.body, data)
            ncats = len(data.categories)
            fully_connected = FullyConnectedNet([2 * nfeats] + layer_sizes + [ncats], drops)
            self.head = nn.Sequential(AdaptiveConcatPool2d(), Flatten(), fully_connected)

        if splits is None:
            body_groups = [self.body]
        elif type(splits) == str:
            body_groups = default_split(arch, self.body)
        elif type(splits) == nn.ModuleList:
            body_groups = [G for G in splits]
        elif type(splits) == list:
            layers = list(self.body.children())
            idxs = [0] + splits + [len(layers)]
            body_groups = [nn.Sequential(*layers[idxs[i]:idxs[i + 1]]) for i in range(len(idxs) - 1)]

        self.layer_groups = body_groups + [self.head]
        self.param_groups = separate_bn_layers(self.layer_groups)

    def forward(self, x_batch):
        return self.head(self.body(x_batch))


class ImageClassificationEnsembleNet(nn.Module):
    "Weighted average of softmax / sigmoid outputs of several classifiers (Vision.py:1339-1373)."

    def __init__(self, models, weights=None, correction='single_label'):
        super().__init__()
        n = len(models)
        self.weights = weights if weights else [1 / n] * n
        self.correction = correction
        self.models = nn.ModuleList(models)
        self.layer_groups = models
        self.param_groups = separate_bn_layers(self.layer_groups)

    def forward(self, x):
        if self.correction == 'single_label':
            return sum(w * F.log_softmax(m(x), dim=1).exp() for w, m in zip(self.weights, self.models))
        if self.correction == 'multi_label':
            return sum(w * m(x).sigmoid() for w, m in zip(self.weights, self.models))


# ---- §6 object detection ------------------------------------------------------------------------------------------

class ObjectDetectionNet(nn.Module):
    """RetinaNet (ResNet-50 + FPN) with re-initialised classifier / regressor heads (Vision.py:1382-1471).
    The reference loads COCO weights from an LFS blob that is not in the repository (retinanet.py:430-435); pass
    `pretrained_path` to load a real checkpoint, otherwise the backbone keeps its seeded random init."""

    def __init__(self, num_classes, ratios=[0.5, 1, 2], scales=[2 ** 0, 2 ** (1 / 3), 2 ** (2 / 3)],
                 prior=0.01, feature_size=256, bn=False, drop=None, pretrained_path=None):
        super().__init__()
        R = vmods.retinanet
        model = R.retinanet(pretrained_path)
        self.layer0 = ResNetBody(model.conv1, model.bn1, model.relu, model.maxpool)
        self.layer1, self.layer2, self.layer3, self.layer4 = model.layer1, model.layer2, model.layer3, model.layer4
        self.resnet = nn.ModuleList([self.layer0, self.layer1, self.layer2, self.layer3, self.layer4])
        self.fpn = model.fpn

        num_anchors = len(ratios) * len(scales)
        self.classifier = R.ClassificationModel(256, num_anchors, num_classes, feature_size, bn, drop)
        self.regressor = R.RegressionModel(256, num_anchors, feature_size, bn, drop)
        self.head = nn.ModuleList([self.classifier, self.regressor])
        R.init_retina_modules(self.head.modules())
        nn.init.constant_(self.classifier.output.weight, 0)
        nn.init.constant_(self.classifier.output.bias, -np.log((1.0 - prior) / prior))
        nn.init.constant_(self.regressor.output.weight, 0)
        nn.init.constant_(self.regressor.output.bias, 0)

        self.layer_groups = [self.resnet, self.fpn, self.head]
        self.param_groups = separate_bn_layers(self.layer_groups)
        self.AnchorGenerator = R.AnchorGenerator(ratios, scales)
        self.BBoxPredictor = R.BBoxPredictor()                    # Vision.py:1444

    def forward(self, x):
        """x [bs,3,H,W] -> [anchors [N,4], reg [bs,N,4], clas [bs,N,num_classes]]"""
        x0 = self.layer0(x)
        x1 = self.layer1(x0)
        x2 = self.layer2(x1)
        x3 = self.layer3(x2)
        x4 = self.layer4(x3)
        features = self.fpn([x2, x3, x4])
        # the head parameters are shared by the five levels: one gradient-sum launch per tensor instead of four autograd adds
        with ops.shared_params([self.regressor, self.classifier], len(features)):
            reg = torch.cat([self.regressor(f) for f in features], dim=1)
            clas = torch.cat([self.classifier(f) for f in features], dim=1)
        return [self.AnchorGenerator(x), reg, clas]


def match_anchors_objects(objects, anchors, pos_thresh=0.5, neg_thresh=0.4):
    """Per-image anchor/object matching (Vision.py:1474-1511): returns pos_idxs, neg_idxs, matches.  Helper API
    (torch ops); the training path uses the fused kernel in SSD_loss."""
    dev = anchors.device
    if len(objects) == 0:
        return (torch.zeros(0, dtype=torch.long, device=dev), torch.arange(len(anchors), device=dev),
                -torch.ones(len(anchors), dtype=torch.long, device=dev))
    max_values, max_idxs = torch.max(jaccard(objects, anchors), dim=0)
    pos = max_values > pos_thresh
    matches = pos.long() * (max_idxs + 1) - 1
    return pos.nonzero().view(-1), (max_values < neg_thresh).nonzero().view(-1), matches


def focal_loss_retina(pred, target, alpha=0.25, gamma=2.0):
    "Focal loss of one image, summed and divided by max(#positives, 1) (Vision.py:1513-1530); helper API."
    p = pred.clamp(1e-4, 1.0 - 1e-4)
    pt = p * target + (1 - p) * (1 - target)
    w = (alpha * target + (1 - alpha) * (1 - target)) * (1 - pt).pow(gamma)
    losses = -w * (target * torch.log(p) + (1 - target) * torch.log(1 - p))
    return losses.sum() / target.sum().clamp(min=1)


def smoothL1_loss_retina(anchs, pred_shift, target):
    "Smooth-L1 (beta = 1/9) on encoded box deltas, mean over n_pos*4 (Vision.py:1532-1566); helper API."
    aw, ah = anchs[:, 2] - anchs[:, 0], anchs[:, 3] - anchs[:, 1]
    ax, ay = anchs[:, 0] + 0.5 * aw, anchs[:, 1] + 0.5 * ah
    tw, th = target[:, 2] - target[:, 0], target[:, 3] - target[:, 1]
    tx, ty = target[:, 0] + 0.5 * tw, target[:, 1] + 0.5 * th
    tw, th = tw.clamp(min=1), th.clamp(min=1)
    true_shift = torch.stack(((tx - ax) / aw, (ty - ay) / ah, torch.log(tw / aw), torch.log(th / ah))).t()
    true_shift = true_shift / torch.tensor([[0.1, 0.1, 0.2, 0.2]], device=anchs.device)
    diff = torch.abs(true_shift - pred_shift)
    losses = 0.5 * 9 * diff.pow(2) * (diff < 1 / 9).float() + (diff - 0.5 / 9) * (diff >= 1 / 9).float()
    return losses.mean()


def ssd1(anchors, bboxes, cats, reg, clas, alpha=0.25, gamma=2.0):
    "(reg_loss, clas_loss) of ONE image (Vision.py:1568-1605) through the fused kernel."
    M = max(len(bboxes), 1)
    B = -torch.ones(1, M, 4, device=reg.device)
    Cc = -torch.ones(1, M, dtype=torch.long, device=reg.device)
    if len(bboxes):
        B[0, :len(bboxes)] = bboxes
        Cc[0, :len(cats)] = cats
    out = ops.retina_loss(anchors, reg.unsqueeze(0), clas.unsqueeze(0), B, Cc, 0.5, alpha, gamma)
    return out[1], out[2]


class SSD_loss(object):
    """(1-beta)*smoothL1 + beta*focal, batch mean of per-image losses (Vision.py:1607-1644).  One fused kernel per
    batch (fwd) + one (bwd); `.reg_loss` / `.clas_loss` are stashed as 0-dim device tensors as in the reference."""

    def __init__(self, beta=0.5, alpha=0.25, gamma=2.0):
        self.beta, self.alpha, self.gamma = beta, alpha, gamma

    def __call__(self, activ, target):
        BBoxes, Cats = target[0], target[1]
        anchors, reg, clas = activ[0], activ[1], activ[2]
        out = ops.retina_loss(anchors, reg, clas, BBoxes, Cats, self.beta, self.alpha, self.gamma)
        self.reg_loss, self.clas_loss = out[1].detach(), out[2].detach()
        return out[0]


class SSD_RegLoss(object):
    "Metric exposing SSD_loss.reg_loss (Vision.py:1646-1654)."
    def __init__(self, loss_func):
        self.loss_func = loss_func

    def __call__(self, pred, target):
        return self.loss_func.reg_loss


class SSD_ClasLoss(object):
    "Metric exposing SSD_loss.clas_loss (Vision.py:1656-1663)."
    def __init__(self, loss_func):
        self.loss_func = loss_func

    def __call__(self, pred, target):
        return self.loss_func.clas_loss


# ---- §6.3 other detection metrics (Vision.py:1666-1800) -------------------------------------------------------------------
class ComputeMaxOverlaps(object):
    """Mean over images of the mean over ground-truth objects of the maximum jaccard overlap with any anchor box — how well
    the anchors cover the objects (Vision.py:1666-1694).  Also accumulates every maximum in self.max_overlaps."""

    def __init__(self):
        self.max_overlaps = []

    def __call__(self, activ, target):
        Objects, anchors, bs = target[0], activ[0], len(target[0])
        batch_means = []
        for i in range(bs):
            objects = Objects[i][Objects[i] >= 0].view(-1, 4)
            if len(objects) == 0:
                continue
            mx = jaccard(objects, anchors).max(dim=1)[0].detach().cpu().numpy()
            self.max_overlaps += list(mx)
            batch_means.append(mx.mean())
        return TEN(np.array(batch_means).mean() if batch_means else 0.0)


def mAP1(targs, preds, scores, thresh):
    """Average precision of one category at one jaccard threshold over a dataset (Vision.py:1696-1747): each ground-truth box
    marks its best-overlapping prediction correct if the overlap exceeds `thresh`; the area under the max-smoothed precision
    curve, divided by the number of ground-truth boxes."""
    from .VisionModels.retinanet import jaccard as np_jaccard
    is_correct, all_scores = [], []
    for t, p, s in zip(targs, preds, scores):
        ok = [0] * len(p)
        if len(p) > 0 and len(t) > 0:
            jac = np_jaccard(np.array(t, dtype=np.float32), np.array(p, dtype=np.float32))
            best = jac.argmax(axis=1)
            for j, k in enumerate(best):
                if jac[j, k] > thresh:
                    ok[int(k)] = 1
        is_correct += ok
        all_scores += list(s)
    ic = np.array([c for _, c in sorted(zip(all_scores, is_correct), reverse=True)])
    ntrue = sum(len(t) for t in targs)
    tp = np.cumsum(ic)
    precision = tp * np.array([1 / n for n in range(1, len(ic) + 1)])
    smoothed = np.flip(np.maximum.accumulate(np.flip(precision)))
    return np.sum(smoothed[ic.nonzero()[0]]) / ntrue


def mAP(predictions, targets, categories, thresholds=COCO_thresholds, verbose=True):
    """Mean average precision over categories and jaccard thresholds (Vision.py:1749-1800).  predictions[i] =
    [pred_boxes, pred_classes, conf_scores] as returned by learner.predict('val'); targets[i] = [(box, category), ...]."""
    N, C = len(predictions), len(categories)
    targs = [[[] for _ in range(N)] for _ in range(C)]
    preds = [[[] for _ in range(N)] for _ in range(C)]
    scores = [[[] for _ in range(N)] for _ in range(C)]
    for i in range(N):
        pred_boxes, pred_classes, conf_scores = predictions[i]
        for j in range(len(pred_boxes)):
            c = pred_classes[j]
            preds[c][i].append(pred_boxes[j])
            scores[c][i].append(conf_scores[j])
        for b, c in targets[i]:
            targs[c][i].append(b)
    vals = np.zeros((len(thresholds), C))
    for c in range(C):
        for j, thresh in enumerate(thresholds):
            vals[j, c] = mAP1(targs[c], preds[c], scores[c], thresh)
            if verbose:
                print('cat =', c, ':', categories[c], ' thresh =', thresh)
                print('cat-thresh mAP = ', vals[j, c])
                print('')
    if verbose:
        print('Overall mAP = ', np.mean(vals))
    return np.mean(vals)


class ImageLearner(Learner):
    """Learner for image data (Vision.py:1803-1812): inherits fit / evaluate / predict unchanged, plus data_resize,
    switch_transform_stats, confusion_matrix and TTA for classification and compute_mAP for object detection.
    Classification (data = ImageDataObj(..., 'single_label' | 'multi_label', ..., get_transforms(...), ...)): the progressive-resizing
    workflow of the Planet notebook — fit at one size, data_resize(sz, bs), fit again, TTA('val') — runs on the device-resident
    images; a resize changes the Transform objects the loaders share with the datasets and uploads nothing.
    With data = ImageDataObj(..., 'bbox', ..., get_transforms_bbox(...), ...) the whole detection workflow runs
    from the public API: fit trains from device_data.DetectionBatches minibatches (a new padded size runs the step eagerly),
    predict('val') divides each image's boxes by its 'scale', TTA_bbox('val', transforms) merges five passes over the resident set,
    compute_mAP scores either (device=True: on the device) and coco_pascal_eval gives the twelve COCO / Pascal numbers without
    pycocotools.  The visualisation helpers (show_images, show_bbox_preds) of the reference's ImageLearner are UI (out of scope,
    SURVEY §2.1 row 12)."""

    def _transforms(self):
        "the Transform objects of the train, val and (if any) test datasets: the ones their loaders read at every minibatch"
        tfms = [self.data.train_ds.transform, self.data.val_ds.transform]
        if self.data.test_ds:
            tfms += [self.data.test_ds.transform]
        return tfms

    def data_resize(self, sz, bs=None):
        """Transform the images to size `sz` from now on, and with `bs` also change the batch size of the loaders (Vision.py:1814-1833),
        'single_label' / 'multi_label' data.  The loaders become views of the resident images (ImageBatches.with_transform: nothing is
        uploaded again; training stays shuffled and sharded by rank); captured steps of the old shape are dropped."""
        if self.data.target_type == 'bbox':
            raise ValueError("data_resize is for 'single_label' / 'multi_label' data: a 'bbox' minibatch has its own padded size")
        if type(sz) == int:
            sz = (sz, sz)
        sz = (int(sz[0]), int(sz[1]))
        tfms = self._transforms()
        if sz[0] != sz[1] and any(t.tfm_type == 'TopDown' for t in tfms):
            raise ValueError("tfm_type='TopDown' rotates by multiples of 90 degrees and needs a square sz (got %r)" % (sz,))
        self.data.sz = sz
        for tfm in tfms:
            tfm.sz = sz
        if bs:
            d = self.data
            d.bs = bs
            tr = d.train_dl
            view = tr._view(tr.transform, bs, True, tr.seed, tr.rank, tr.world)
            view.epoch = tr.epoch                       # the epoch permutations go on, they do not start over
            d.train_dl = view
            d.val_dl = d.val_dl.with_transform(d.val_dl.transform, bs)
            if d.test_dl:
                d.test_dl = d.test_dl.with_transform(d.test_dl.transform, bs)
        self._graphs = {}

    def switch_transform_stats(self, new_stats):
        "Normalise with `new_stats` = [mean, std] from now on, in the train, val and test transforms (Vision.py:1835-1844)."
        for tfm in self._transforms():
            tfm.stats = new_stats

    def confusion_matrix(self, pred_labels=None):
        "Plot the confusion matrix of the validation set, 'single_label' only; predict('val') if no labels are given (Vision.py:1846-1857)."
        if self.target_type != 'single_label':
            raise ValueError("confusion_matrix works only with target_type 'single_label' (got %r)" % (self.target_type,))
        from sklearn.metrics import confusion_matrix
        true_labels = self.data.val_ds.y
        if pred_labels is None:
            pred_probs, pred_labels = self.predict('val')
        cm = confusion_matrix(true_labels, pred_labels)
        classes = {self.data.categories[x]: x for x in self.data.categories}
        plot_confusion_matrix(cm, classes)

    def tta_transforms(self, beta=0.4):
        """([tfm0 .. tfm4], weights) of TTA (Vision.py:2014-2023, 2033): the evaluation transform and four light augmentations (rotation
        up to 5 degrees, no zoom) cropped at 0, 1/3, 2/3 and the end of the longer side; type, stats and size of the TRAIN transform."""
        tfm = self.data.train_ds.transform
        tfm_type, stats, sz = tfm.tfm_type, tfm.stats, tfm.sz
        tfms = [Transform('Basic', 'center', None, sz, None, None, None, None, stats=stats)]
        tfms += [Transform(tfm_type, c, None, sz, 5, 1.0, stats=stats) for c in (0.0, 0.33, 0.67, 1.0)]
        return tfms, [beta] + [(1 - beta) / 4] * 4

    def TTA(self, ds_type, beta=0.4):
        """Test-time augmentation of the 'val' or 'test' set, 'single_label' / 'multi_label' (Vision.py:1983-2034): predictions under
        the five transforms of `tta_transforms`, combined with weights beta, (1 - beta) / 4 x 4; returns what combine_preds returns
        (probabilities [n, ncat], labels).  The five loaders are views of the one resident copy of the set; view k draws its
        rotations, flips and lighting from RandomState(loader seed + k) (the reference's draws are unseeded)."""
        if self.target_type not in ('single_label', 'multi_label'):
            raise ValueError("TTA works only with target_type 'single_label' or 'multi_label' (got %r)" % (self.target_type,))
        if ds_type not in ('val', 'test'):
            raise ValueError("ds_type must be 'val' or 'test' (got %r)" % (ds_type,))
        dl = self.data.val_dl if ds_type == 'val' else self.data.test_dl
        tfms, weights = self.tta_transforms(beta)
        preds = [self.predict(dl.with_transform(tfm, bs=self.data.bs, seed=dl.seed + k))[0] for k, tfm in enumerate(tfms)]
        return combine_preds(preds, self.target_type, weights)

    TTA_BBOX_PASSES = 5

    def TTA_bbox(self, ds_type, transforms, thresh=0.05, max_overlap=0.5, rel_thresh=None, top_k=1000, max_boxes=20, dup=None, inc=None):
        """Test-time augmentation of the 'val' or 'test' set, target_type 'bbox' (Vision.py:2036-2121): five passes over the set at batch
        size 1 in dataset order — transforms[0] (tfm_eval) once, transforms[1] (tfm_aug) four times — each through BBoxPredictor with
        the given arguments; every pass's boxes are mapped back to the original image (minus the jitter, times 1 / (rand_scale scale),
        un-mirrored), the five lists of an image are concatenated in pass order and nms(...) runs once more on the union.  Returns what
        predict('val') returns: [boxes, classes, scores] per image, so compute_mAP(predictions=learner.TTA_bbox('val', transforms)).
        The passes are views of the one resident copy of the set (DetectionBatches.with_transform); the undo and the concatenation
        are one kernel (ops.tta_bbox_merge) and the final NMS one batched nnl_nms over all images.  With rel_thresh, dup and inc all
        None the only list filter is the max_boxes cut, and every (pass, image) leaves its first max_boxes survivors on the device:
        no device->host copy and no synchronisation until the one copy of the final result.  With any of the three set, each (pass,
        image) goes through BBoxPredictor.__call__ as in predict and the pruned lists are uploaded once.
        Three deliberate differences from the reference:
          * every pass clips its boxes to the part of the padded, jittered minibatch that IS the image, [col_jit, col_jit + rw] x
            [row_jit, row_jit + rh] (nnl_bbox_decode_window), so every returned box lies inside its original image (short of it by at
            most the int() truncation of the resize); the reference, and predict, clip to the padded minibatch, whose padding of up to
            31 pixels and whose jitter border map to places outside the image.  TTA_bbox under identity passes therefore equals
            predict exactly when the eval minibatch needs no padding, and differs from it only in boxes that reach into the padding;
          * a pass un-mirrors only the images it mirrored ('SideOn' and a flip draw of 1, the NNL_IMAGE_AUG_FLIP flag of batch_table);
            the reference un-mirrors passes 1-4 on the draw alone, which mirrors the correct boxes of a 'Basic' tfm_aug;
          * pass k draws its per-image values from RandomState(loader seed + k) through TransformBBox.sample, one draw per image in
            dataset order (at batch size 1 every image is its minibatch's first, so its own rand_scale and jitter apply); the
            reference pre-draws unseeded lists (get_values)."""
        from ..General.Learner import _raise_if_index_error
        from .VisionModels.retinanet import _device_nms_kept, _kept_to_host, _prune
        if self.target_type != 'bbox':
            raise ValueError("TTA_bbox works only with target_type 'bbox' (got %r)" % (self.target_type,))
        if ds_type not in ('val', 'test'):
            raise ValueError("ds_type must be 'val' or 'test' (got %r)" % (ds_type,))
        dl = self.data.val_dl if ds_type == 'val' else self.data.test_dl
        if dl is None:
            raise ValueError("TTA_bbox('test', ...) needs a test set: the data object has none")
        if not (isinstance(transforms, (list, tuple)) and len(transforms) == 2 and all(isinstance(t, TransformBBox) for t in transforms)):
            raise ValueError('transforms must be [tfm_eval, tfm_aug], two TransformBBox (get_transforms_bbox)')
        P, L = self.TTA_BBOX_PASSES, dl.n
        views = [dl.with_transform(transforms[0] if k == 0 else transforms[1], bs=1, seed=dl.seed + k) for k in range(P)]
        on_device = rel_thresh is None and dup is None and inc is None
        predictor, dev = self.model.BBoxPredictor, dl.device
        self.model.eval()
        with torch.no_grad():
            if on_device:
                M = max(1, int(top_k) if max_boxes is None else min(int(max_boxes), int(top_k)))
                limit = M if max_boxes is None else int(max_boxes)           # max_boxes 0: slots exist, counts are 0
                boxes = torch.zeros(L, P, M, 4, dtype=torch.float32, device=dev)
                classes = torch.zeros(L, P, M, dtype=torch.int32, device=dev)
                scores = torch.zeros(L, P, M, dtype=torch.float32, device=dev)
                counts = torch.zeros(L, P, dtype=torch.int32, device=dev)
            else:
                lists = [[None] * P for _ in range(L)]
            for k, view in enumerate(views):
                for j, (x_batch, _) in enumerate(view):
                    x_batch = to_cuda(x_batch)
                    y_pred = self.predict1minibatch(x_batch)
                    if isinstance(y_pred, tuple):
                        y_pred = y_pred[0]
                    anchors, reg, clas = y_pred
                    d = view.last_draws[j]                                      # the part of the padded minibatch that is the image
                    window = (d['col_jit'], d['row_jit'], d['col_jit'] + d['rw'], d['row_jit'] + d['rh'])
                    if on_device:
                        kb, kc, ks, kn = predictor.survivors_on_device(x_batch, reg, clas, anchors, thresh, max_overlap, top_k, window)
                        m = min(kb.shape[1], M)                                 # rows past kept_count are uninitialised memory (torch.empty in
                        # _device_nms_kept) and are copied as they are: `counts` guards every read of the table, in the merge kernel too
                        boxes[j, k, :m], classes[j, k, :m], scores[j, k, :m] = kb[0, :m], kc[0, :m], ks[0, :m]
                        torch.clamp(kn, max=min(m, limit), out=counts[j, k:k + 1])
                    else:
                        B, Cl, Sc = predictor(x_batch, reg, clas, anchors, thresh, max_overlap, rel_thresh, top_k, max_boxes, dup, inc, window)
                        lists[j][k] = (B[0], Cl[0], Sc[0])
            if not on_device:                                               # the pruned lists, packed into the same table: one upload
                M = max(1, max(len(lists[j][k][0]) for j in range(L) for k in range(P)))
                hb, hc = np.zeros((L, P, M, 4), dtype=np.float32), np.zeros((L, P, M), dtype=np.int32)
                hs, hn = np.zeros((L, P, M), dtype=np.float32), np.zeros((L, P), dtype=np.int32)
                for j in range(L):
                    for k in range(P):
                        B, Cl, Sc = lists[j][k]
                        n = hn[j, k] = len(B)
                        if n:
                            hb[j, k, :n], hc[j, k, :n], hs[j, k, :n] = np.stack(B), np.asarray(Cl), np.asarray(Sc)
                boxes, classes, scores, counts = (torch.from_numpy(a).to(dev) for a in (hb, hc, hs, hn))
            cols = [W for _, W in dl.shapes]
            undo = np.stack([ops.tta_undo_rows(view.last_draws, dl.scales, cols) for view in views], axis=1)        # [L, P]
            undo = torch.from_numpy(np.ascontiguousarray(undo).view(np.uint8).reshape(L, P, ops.TTA_UNDO.itemsize)).to(dev)
            merged = []
            for a in range(0, L, 32768):                                    # nnl_nms takes fewer than 65536 images per call
                z = min(a + 32768, L)
                cand = ops.tta_bbox_merge(boxes[a:z], classes[a:z], scores[a:z], counts[a:z], undo[a:z])
                merged.append((_device_nms_kept(cand, z - a, P * M, top_k, max_overlap, dev), z - a))
            out = []
            for kept, n in merged:
                for b, c, s in _kept_to_host(kept, n):
                    out.append(list(_prune(list(b), list(c), list(s), rel_thresh, max_boxes, dup, inc)) if len(b) else [[], [], []])
        _raise_if_index_error(local=True)
        return out

    def compute_mAP(self, predictions=None, thresh=0.05, max_overlap=0.5, rel_thresh=None, top_k=1000, max_boxes=20,
                    dup=None, inc=None, mAP_thresholds=COCO_thresholds, device=False):
        """mAP of the validation set, target_type 'bbox' only (Vision.py:2123-2140).  device=True scores on the device (mAP_device:
        the same numbers up to the summation order of each curve); the default is the host loop."""
        categories, targets = self.data.categories, self.data.val_ds.y
        if predictions is None:
            predictions = self.predict('val', True, thresh, max_overlap, rel_thresh, top_k, max_boxes, dup, inc)
        if device:
            return mAP_device(predictions, targets, categories, mAP_thresholds)
        return mAP(predictions, targets, categories, mAP_thresholds)

    def coco_pascal_eval(self, val_json, predictions=None, thresh=0.05, max_overlap=0.5, rel_thresh=None, top_k=1000, max_boxes=20,
                         dup=None, inc=None, cat2dscat=None, save_preds=False):
        """The COCO / Pascal evaluation of the validation set's box predictions (Vision.py:2142-2177): what pycocotools'
        COCOeval(coco_true, coco_pred, 'bbox') evaluate / accumulate / summarize compute with Params.setDetParams (iouThrs
        linspace(.5, .95, 10), recThrs linspace(0, 1, 101), maxDets [1, 10, 100], the four area ranges), without pycocotools: the
        per-(image, category) matching and the per-(category, area, maxDets, threshold) curves are HIP kernels (ops.det_eval_coco,
        K14) and the twelve summary numbers are numpy means over the arrays that come back.  Only iouType 'bbox' with useCats = 1.
        val_json: path of the annotation file, or the loaded dict.  predictions: as predict('val') returns them, or None to predict
        with the other arguments.  Image ids are self.data.val_ds.images[i]['id']; the category map is `cat2dscat`, else
        self.data.cat2dscat, else {i: categories[i]['id']} in the json's order (as from_json_bbox builds it, Vision.py:1120).
        Deliberate differences from the reference:
          * it RETURNS the twelve numbers (AP, AP50, AP75, AP small / medium / large, AR at 1 / 10 / 100 detections, AR small /
            medium / large) as a float64 vector; the reference returns None.  They are printed in summarize's format when
            Learner.verbose;
          * precision [T, R, K, A, M], recall [T, K, A, M], scores and the parameters are kept in self.coco_eval;
          * preds.json is written (to self.PATH) only with save_preds=True;
          * ValueError, before anything is uploaded, for: an annotation id of 0 (COCOeval stores matched ids and tests `== 0` for
            "unmatched", so such a ground truth matches and still counts as a false positive there; we store positions + 1), a
            validation image without 'id', a prediction category absent from the map, and no prediction at all (the reference's
            loadRes fails on anns[0])."""
        import json
        if self.target_type != 'bbox':
            raise ValueError("coco_pascal_eval works only with target_type 'bbox' (got %r)" % (self.target_type,))
        coco = val_json
        if not isinstance(coco, dict):
            with open(val_json) as f:
                coco = json.load(f)
        images = self.data.val_ds.images
        missing = [i for i, im in enumerate(images) if not (isinstance(im, dict) and 'id' in im)]
        if missing:
            raise ValueError("coco_pascal_eval: validation image %d has no 'id'" % missing[0])
        if cat2dscat is None:
            cat2dscat = getattr(self.data, 'cat2dscat', None)
        if cat2dscat is None:
            cat2dscat = {i: c['id'] for i, c in enumerate(coco['categories'])}
        if predictions is None:
            predictions = self.predict('val', True, thresh, max_overlap, rel_thresh, top_k, max_boxes, dup, inc)
        if len(predictions) != len(images):
            raise ValueError('coco_pascal_eval: %d prediction lists for %d validation images' % (len(predictions), len(images)))
        if sum(len(p[0]) for p in predictions) == 0:
            raise ValueError('coco_pascal_eval: there is no prediction at all')
        image_ids = [im['id'] for im in images]
        iouThrs, recThrs, maxDets = np.linspace(.5, .95, 10), np.linspace(0, 1, 101), [1, 10, 100]      # Params.setDetParams
        areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        areaRngLbl = ['all', 'small', 'medium', 'large']
        packed = ops.det_eval_pack(predictions, coco=coco, image_ids=image_ids, cat2dscat=cat2dscat, max_det=maxDets[-1])
        if save_preds:
            rows = []
            for ID, (B, Cl, Sc) in zip(image_ids, predictions):
                for box, cat, score in zip(B, Cl, Sc):
                    rows.append({'image_id': ID, 'category_id': cat2dscat[int(cat)], 'score': float(score),
                                 'bbox': [float(box[0]), float(box[1]), float(box[2] - box[0]), float(box[3] - box[1])]})
            with open(self.PATH + 'preds.json', 'w') as f:
                json.dump(rows, f, indent=4)
        precision, recall, scores = ops.det_eval_coco(packed, iouThrs, recThrs, maxDets, areaRng, device=default_device())
        self.coco_eval = {'precision': precision, 'recall': recall, 'scores': scores, 'iouThrs': iouThrs, 'recThrs': recThrs,
                          'maxDets': maxDets, 'areaRng': areaRng, 'areaRngLbl': areaRngLbl, 'catIds': packed['cat_ids'],
                          'imgIds': packed['img_ids']}
        stats, lines = coco_summarize(precision, recall, iouThrs, maxDets, areaRngLbl)
        self.coco_eval['stats'] = stats
        if Learner.verbose:
            print('\n'.join(lines))
        return stats


def coco_summarize(precision, recall, iouThrs, maxDets, areaRngLbl):
    """The twelve numbers of COCOeval.summarize for detections (cocoeval.py:430-480) and their printed lines: each the mean of the
    entries above -1 of a slice of precision [T, R, K, A, M] or recall [T, K, A, M], -1 if there is none."""
    def one(ap, iouThr, area, max_det):
        a, m = areaRngLbl.index(area), list(maxDets).index(max_det)
        s = precision if ap else recall
        if iouThr is not None:
            s = s[np.where(iouThr == iouThrs)[0]]
        s = s[..., a, m]
        mean = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        iou = '{:0.2f}:{:0.2f}'.format(iouThrs[0], iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
        line = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
            'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, area, max_det, mean)
        return mean, line
    top = maxDets[2]
    rows = [(1, None, 'all', top), (1, .5, 'all', top), (1, .75, 'all', top), (1, None, 'small', top), (1, None, 'medium', top),
            (1, None, 'large', top), (0, None, 'all', maxDets[0]), (0, None, 'all', maxDets[1]), (0, None, 'all', top),
            (0, None, 'small', top), (0, None, 'medium', top), (0, None, 'large', top)]
    got = [one(*r) for r in rows]
    return np.array([g[0] for g in got], dtype=np.float64), [g[1] for g in got]


def mAP_device(predictions, targets, categories, thresholds=COCO_thresholds, verbose=True):
    """`mAP` on the device: the per-(category, image) overlaps and arg-max marks and the per-(category, threshold) curves are HIP
    kernels (ops.det_map, K14) instead of one Python iteration per (category, threshold, image).  Prints what mAP prints and returns
    its mean; a value differs from mAP's only by the order in which a curve's non-negative terms are added.  ValueError for a
    ground-truth box of non-positive area, whose 0 / 0 overlap the host path turns into a NaN arg-max."""
    C = len(categories)
    packed = ops.det_eval_pack(predictions, targets=targets, n_categories=C)
    vals = ops.det_map(packed, thresholds, device=default_device())
    if verbose:
        for c in range(C):
            for j, thresh in enumerate(thresholds):
                print('cat =', c, ':', categories[c], ' thresh =', thresh)
                print('cat-thresh mAP = ', vals[j, c])
                print('')
        print('Overall mAP = ', np.mean(vals))
    return np.mean(vals)
