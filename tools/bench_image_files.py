"""Image datasets from files on the GPU box: what the first cell of a vision notebook costs.  The tool writes its own set of PNG or
JPEG files into a temporary directory (smooth content plus noise, so that the files compress like photographs rather than like
noise) and measures
  (1) decode + upload: device_data.ImageStore.from_files for each thread count, images/s and decoded MB/s;
  (2) ops.image_stats' kernel (nnl_image_stats) with HIP events over the resident set, against its read-once bound of
      arena bytes / 6.29 TB/s (DESIGN.md's measured device copy rate);
  (3) nnl_image_resize_u8 with HIP events: the whole set to --presize (shorter side), against read + write of both arenas;
  (4) Vision.get_stats end to end (decode, upload, kernel, read-back) against a host baseline written here that decodes the same
      files with the same decoder on the same number of threads and reduces every image in float32, as the reference's get_stats
      does; and what share of get_stats is host decode.
Every wall-clock figure is the median of three alternations of the variants in one process after one warm-up pass, with the spread
(min .. max); kernel figures are medians of three event-timed loops.
Usage: python tools/bench_image_files.py [--images 256] [--height 375] [--width 500] [--format png|jpeg] [--threads 1,4,8,16]
                                         [--presize 224]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import device_data, ops  # noqa: E402
from neuralnetworklibrary_amd._lib import check, lib, ptr, stream  # noqa: E402
from neuralnetworklibrary_amd.Applications import Vision as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--images', type=int, default=256)
ap.add_argument('--height', type=int, default=375)
ap.add_argument('--width', type=int, default=500)
ap.add_argument('--format', choices=['png', 'jpeg'], default='jpeg')
ap.add_argument('--threads', default='1,4,8,16')
ap.add_argument('--presize', type=int, default=224)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
COPY_TBS = 6.29
THREADS = [int(t) for t in a.threads.split(',')]


def write_files(root):
    from PIL import Image
    rs = np.random.RandomState(0)
    paths = []
    yy, xx = np.mgrid[0:a.height + 40, 0:a.width + 40].astype(np.float32)
    for i in range(a.images):
        h, w = a.height + int(rs.randint(-40, 41)), a.width + int(rs.randint(-40, 41))
        f = rs.uniform(0.01, 0.06, size=(3, 2)).astype(np.float32)
        img = np.stack([127 + 100 * np.sin(f[c, 0] * yy[:h, :w] + i) * np.cos(f[c, 1] * xx[:h, :w]) for c in range(3)], axis=2)
        img = np.clip(img + rs.normal(0, 6, size=img.shape), 0, 255).astype(np.uint8)
        p = os.path.join(root, 'img%05d.%s' % (i, 'png' if a.format == 'png' else 'jpg'))
        Image.fromarray(img).save(p, **({'quality': 90} if a.format == 'jpeg' else {}))
        paths.append(p)
    return paths


def med(values):
    return {'median': round(float(np.median(values)), 4), 'min': round(float(min(values)), 4), 'max': round(float(max(values)), 4)}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def events_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def host_get_stats(paths, threads):
    "the reference's get_stats on the host: per image float32 img / 255, mean and mean of squares, averaged in fp64"
    def one(p):
        img = device_data.decode_image_u8(p).astype(np.float32) / 255
        return img.mean(axis=(0, 1)), (img ** 2).mean(axis=(0, 1))
    with ThreadPoolExecutor(max_workers=threads) as pool:
        parts = list(pool.map(one, paths))
    means = np.sum([m for m, _ in parts], axis=0, dtype=np.float64) / len(paths)
    second = np.sum([s for _, s in parts], axis=0, dtype=np.float64) / len(paths)
    return [means, np.sqrt(second - means ** 2)]


result = {'images': a.images, 'format': a.format, 'size': [a.height, a.width], 'threads': THREADS}
with tempfile.TemporaryDirectory() as root:
    paths = write_files(root)
    result['file_MB'] = round(sum(os.path.getsize(p) for p in paths) / 1e6, 2)

    # ---- (1) decode + upload ------------------------------------------------------------------------------------------
    store = device_data.ImageStore.from_files(paths, threads=THREADS[-1])          # warm-up: file cache, Pillow, pinned allocation
    arena_bytes = store.arena.numel()
    result['arena_MB'] = round(arena_bytes / 1e6, 2)
    runs = {t: [] for t in THREADS}
    for _ in range(3):
        for t in THREADS:
            runs[t].append(wall(lambda: device_data.ImageStore.from_files(paths, threads=t))[0])
    result['decode_upload'] = {}
    for t in THREADS:
        m = med(runs[t])
        result['decode_upload'][t] = dict(m, images_per_s=round(a.images / m['median'], 1), MB_per_s=round(arena_bytes / 1e6 / m['median'], 1))
        print('decode + upload, %2d threads: %.3f s (%.3f .. %.3f)  %.0f images/s  %.0f MB/s decoded'
              % (t, m['median'], m['min'], m['max'], a.images / m['median'], arena_bytes / 1e6 / m['median']), flush=True)

    # ---- (2) nnl_image_stats ------------------------------------------------------------------------------------------
    out = torch.empty(len(store), 6, dtype=torch.int64, device=store.arena.device)
    stats_call = lambda: check(lib.nnl_image_stats(ptr(store.arena), arena_bytes, ptr(store.desc), len(store), 0, len(store), ptr(out), stream()))
    for _ in range(5):
        stats_call()
    us = med([events_us(stats_call, 50) for _ in range(3)])
    bound_us = arena_bytes / (COPY_TBS * 1e6)
    result['image_stats'] = dict(us, bound_us=round(bound_us, 2), fraction_of_bound=round(bound_us / us['median'], 3))
    print('nnl_image_stats: %.1f us (%.1f .. %.1f) for %.1f MB; read-once bound %.1f us -> %.0f %% of the bound'
          % (us['median'], us['min'], us['max'], arena_bytes / 1e6, bound_us, 100 * bound_us / us['median']), flush=True)

    # ---- (3) nnl_image_resize_u8 ----------------------------------------------------------------------------------------
    small = [device_data.presize_shape(h, w, a.presize) for h, w in store.shapes]
    ddesc_host, dst_bytes = device_data._desc_table(small)
    ddesc = torch.from_numpy(ddesc_host).to(store.arena.device)
    dst = torch.empty(dst_bytes, dtype=torch.uint8, device=store.arena.device)
    resize_call = lambda: ops.image_resize_u8(store.arena, store.desc, ddesc, dst)
    for _ in range(5):
        resize_call()
    us = med([events_us(resize_call, 50) for _ in range(3)])
    bound_us = (arena_bytes + dst_bytes) / (COPY_TBS * 1e6)
    result['image_resize_u8'] = dict(us, dst_MB=round(dst_bytes / 1e6, 2), bound_us=round(bound_us, 2), fraction_of_bound=round(bound_us / us['median'], 3))
    print('nnl_image_resize_u8 to shorter side %d: %.1f us (%.1f .. %.1f), %.1f MB -> %.1f MB; read + write bound %.1f us -> %.0f %% of the bound'
          % (a.presize, us['median'], us['min'], us['max'], arena_bytes / 1e6, dst_bytes / 1e6, bound_us, 100 * bound_us / us['median']), flush=True)

    # ---- (4) get_stats end to end ----------------------------------------------------------------------------------------
    T = min(16, int(os.environ.get('NNL_DECODE_THREADS', 8)))
    V.get_stats(root), host_get_stats(paths, T)                                     # warm-up of both
    runs = {'device': [], 'host': [], 'decode_only': []}

    def decode_only():
        with ThreadPoolExecutor(max_workers=T) as pool:
            list(pool.map(lambda p: device_data.decode_image_u8(p).shape, paths))
    for _ in range(3):
        t_dev, got = wall(lambda: V.get_stats(root))
        t_host, want = wall(lambda: host_get_stats(paths, T))
        runs['device'].append(t_dev), runs['host'].append(t_host), runs['decode_only'].append(wall(decode_only)[0])
    dv, hs, dc = med(runs['device']), med(runs['host']), med(runs['decode_only'])
    result['get_stats'] = {'threads': T, 'device_s': dv, 'host_float32_s': hs, 'decode_only_s': dc,
                           'decode_share_of_device': round(dc['median'] / dv['median'], 3), 'speedup': round(hs['median'] / dv['median'], 3),
                           'max_abs_diff_mean': float(np.abs(got[0] - want[0]).max()), 'max_abs_diff_std': float(np.abs(got[1] - want[1]).max())}
    print('get_stats, %d threads: ImageStore + kernel %.3f s (%.3f .. %.3f); host float32 baseline %.3f s (%.3f .. %.3f); decode alone %.3f s '
          '= %.0f %% of the device path' % (T, dv['median'], dv['min'], dv['max'], hs['median'], hs['min'], hs['max'], dc['median'],
                                            100 * dc['median'] / dv['median']), flush=True)
print(json.dumps(result))
