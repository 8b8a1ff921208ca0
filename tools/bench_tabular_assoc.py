"""associations_pairs at the Rossmann shape: `--rows` rows (1 050 330), 20 categorical columns with cardinalities from 2 to 1115 (Store x
DayOfYear is the 1115 x 366 table), 16 continuous columns, 3 % missing values everywhere.  Three modes: cat x cat (400 pairs,
mutual_info_symmetric), cat x cont (320 pairs, correlation_ratio) and cont x cont (256 pairs, abs_max_correlation).

Reported per mode (medians over `--rounds` alternations with baseline (b), after one warm-up of everything; spread = max - min):
  host_ms     factorise / convert the distinct columns + the ONE upload                   (host clock around a device synchronise)
  kernel_ms   the ops.assoc_* calls between HIP events, next to the traffic bound: every needed column read ONCE per pass over the
              6.29 TB/s copy rate (the kernels read a column once per chunk of pairs, so this bound is not theirs to reach)
  back_ms     the copy back of the per-pair numbers + the returned frame
  total_ms    the public call, end to end
Baselines, written here:
  (a) `per_pair_pandas`: what the notebook does, per ordered pair: filter the frame, then crosstab / groupby / four corr.  Timed on
      the first `--pandas-pairs` off-diagonal pairs of each mode and EXTRAPOLATED to all off-diagonal pairs (labelled so).
  (b) `numpy`: the same numbers from numpy arrays without pandas, one pair at a time but vectorised over the rows (np.bincount on
      combined codes, weighted bincounts, masked dot products), on factorised columns that are prepared ONCE (its factorise time is
      reported, and counted in its total).  It needs no device.  Checked against ours before anything is timed.
Run it under a time limit of its own, e.g. `timeout 1100 python tools/bench_tabular_assoc.py`.
Usage: python tools/bench_tabular_assoc.py [--rows 1050330] [--rounds 3] [--pandas-pairs 3]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd.Applications import StructuredData as SD  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=1050330)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--pandas-pairs', type=int, default=3)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
warnings.simplefilter('ignore')
HBM = 6.29e12
CARDS = [1115, 366, 2, 2, 3, 4, 4, 7, 7, 12, 12, 22, 25, 31, 31, 52, 52, 3, 3, 2]
N_CONT = 16
MODES = {'cat_x_cat': ('cat', 'mutual_info_symmetric'), 'cat_x_cont': ('cat_cont', 'correlation_ratio'),
         'cont_x_cont': ('cont', 'abs_max_correlation')}

rs = np.random.RandomState(0)
n = a.rows
cols = {}
for k, c in enumerate(CARDS):
    v = rs.randint(0, c, n).astype('float64')
    v[rs.random_sample(n) < 0.03] = np.nan
    cols['c%02d' % k] = v
for k in range(N_CONT):
    v = rs.standard_normal(n) * (1 + k) + 100 * k + (0.2 * np.nan_to_num(cols['c%02d' % (2 + k % 8)]) if k % 2 else 0.0)
    v[rs.random_sample(n) < 0.03] = np.nan
    cols['x%02d' % k] = v
df = pd.DataFrame(cols)
CAT, CONT = ['c%02d' % k for k in range(len(CARDS))], ['x%02d' % k for k in range(N_CONT)]


def mode_vars(family):
    return {'cat': (CAT, None), 'cont': (None, CONT), 'cat_cont': (CAT, CONT)}[family]


def mode_pairs(family):
    rows, cs = {'cat': (CAT, CAT), 'cont': (CONT, CONT), 'cat_cont': (CAT, CONT)}[family]
    return rows, cs, [(x, y) for x in rows for y in cs]


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def phases(family, Type):
    "the public call phase by phase, through the same helpers"
    rows, cs, pairs = mode_pairs(family)
    todo = [p for p in pairs if p[0] != p[1]]
    h, prepared = clock(lambda: SD._assoc_prepare(df, todo, family))
    k, out = device_ms(lambda: SD._assoc_run(prepared, family, with_abs=True))

    def back():
        st = out.cpu().numpy()
        return pd.DataFrame(np.zeros((len(rows), len(cs))), index=rows, columns=cs), st
    b, _ = clock(back)
    return h, k, b


# ---- baseline (a): per pair, pandas, as the notebook does ------------------------------------------------------------------

def pandas_pair(X, Y, family):
    D = df[df[X].notnull() & df[Y].notnull()][[X, Y]]
    if len(D) == 0 or len(D[X].value_counts()) == 1 or len(D[Y].value_counts()) == 1:
        return 0.0
    if family == 'cat':
        def ent(v):
            p = D[v].value_counts() / len(D)
            return -np.sum(np.log(p) * p)
        f = np.array(pd.crosstab(D[X], D[Y])).flatten()
        p = np.maximum(f / f.sum(), 1e-20)
        hx, hy, hxy = ent(X), ent(Y), -np.sum(np.log(p) * p)
        return 0.5 * ((hx + hy - hxy) / hx + (hx + hy - hxy) / hy)
    if family == 'cat_cont':
        mean, var = D[Y].mean(), D[Y].var()
        g = D.groupby(X)[Y]
        means, counts = g.mean(), g.count()
        return np.sqrt((counts * (means - mean) ** 2).sum() / counts.sum() / var)
    x, y = D[X], D[Y]
    x2, y2 = (x - x.mean()).abs(), (y - y.mean()).abs()
    return max(abs(x.corr(y)), abs(x.corr(y2)), abs(x2.corr(y)), abs(x2.corr(y2)))


# ---- baseline (b): numpy, vectorised over the rows --------------------------------------------------------------------------

def numpy_prepare(family):
    codes = {c: pd.factorize(df[c])[0] for c in CAT} if family != 'cont' else {}
    card = {c: int(v.max()) + 1 for c, v in codes.items()}
    vals = {c: df[c].to_numpy(dtype='float64') for c in CONT} if family != 'cat' else {}
    return codes, card, vals


def numpy_all(family, prepared):
    codes, card, vals = prepared
    rows, cs, pairs = mode_pairs(family)
    out = np.zeros(len(pairs))
    for k, (X, Y) in enumerate(pairs):
        if X == Y:
            out[k] = 1.0
        elif family == 'cat':
            cx, cy = codes[X], codes[Y]
            ok = (cx >= 0) & (cy >= 0)
            t = np.bincount(cx[ok].astype(np.int64) * card[Y] + cy[ok], minlength=card[X] * card[Y]).reshape(card[X], card[Y])
            m = t.sum()
            r, c = t.sum(1), t.sum(0)
            if m == 0 or (r > 0).sum() == 1 or (c > 0).sum() == 1:
                continue

            def ent(f):
                p = f[f > 0] / m
                return -np.sum(np.log(p) * p)
            empty = (r > 0).sum() * (c > 0).sum() - (t > 0).sum()
            hx, hy, hxy = ent(r), ent(c), ent(t.ravel()) - empty * 1e-20 * np.log(1e-20)
            out[k] = 0.5 * ((hx + hy - hxy) / hx + (hx + hy - hxy) / hy)
        elif family == 'cat_cont':
            cx, y = codes[X], vals[Y]
            ok = (cx >= 0) & ~np.isnan(y)
            cx, y = cx[ok], y[ok]
            if len(y) == 0 or y.min() == y.max():
                continue
            cnt, s1 = np.bincount(cx, minlength=card[X]), np.bincount(cx, weights=y, minlength=card[X])
            if (cnt > 0).sum() == 1:
                continue
            mean = y.mean()
            d = s1[cnt > 0] / cnt[cnt > 0] - mean
            out[k] = np.sqrt((cnt[cnt > 0] * d * d).sum() / len(y) / y.var(ddof=1))
        else:
            x, y = vals[X], vals[Y]
            ok = ~np.isnan(x) & ~np.isnan(y)
            x, y = x[ok], y[ok]
            if len(x) == 0 or x.min() == x.max() or y.min() == y.max():
                continue
            dx, dy = x - x.mean(), y - y.mean()
            ax, ay = np.abs(dx), np.abs(dy)
            ax, ay = ax - ax.mean(), ay - ay.mean()
            sxx, syy, saa, sbb = dx @ dx, dy @ dy, ax @ ax, ay @ ay
            out[k] = max(abs(dx @ dy) / np.sqrt(sxx * syy), abs(dx @ ay) / np.sqrt(sxx * sbb), abs(ax @ dy) / np.sqrt(saa * syy),
                         abs(ax @ ay) / np.sqrt(saa * sbb))
    return out.reshape(len(rows), len(cs))


stat = lambda v: {'median': float(np.median(v)), 'spread': float(max(v) - min(v))}  # noqa: E731
report = {'rows': n, 'rounds': a.rounds, 'categorical': len(CAT), 'continuous': len(CONT), 'cardinalities': CARDS}
for mode, (family, Type) in MODES.items():
    cat_vars, cont_vars = mode_vars(family)
    rows, cs, pairs = mode_pairs(family)
    # correctness, which also warms everything up
    ours = SD.associations_pairs(df, Type, cat_vars=cat_vars, cont_vars=cont_vars, plot=False)
    prepared = numpy_prepare(family)
    want = numpy_all(family, prepared)
    err = float(np.abs(ours.to_numpy() - want).max())
    assert err < 1e-9, (mode, err)
    phases(family, Type)
    T = {k: [] for k in ('host', 'kernel', 'back', 'total', 'numpy_prepare', 'numpy_pairs')}
    for _ in range(a.rounds):
        t0, prepared = clock(lambda: numpy_prepare(family))
        T['numpy_prepare'].append(t0)
        T['numpy_pairs'].append(clock(lambda: numpy_all(family, prepared))[0])
        T['total'].append(clock(lambda: SD.associations_pairs(df, Type, cat_vars=cat_vars, cont_vars=cont_vars, plot=False))[0])
        h, k, b = phases(family, Type)
        T['host'].append(h); T['kernel'].append(k); T['back'].append(b)
    off = [p for p in pairs if p[0] != p[1]]
    sample = off[:a.pandas_pairs]
    t_pandas, got = clock(lambda: [pandas_pair(X, Y, family) for X, Y in sample])
    for (X, Y), g in zip(sample, got):
        assert abs(g - ours.loc[X, Y]) < 1e-9, (mode, X, Y, g, ours.loc[X, Y])
    passes = 2 if family == 'cont' else 1
    col_bytes = {'cat': 4 * len(CAT), 'cont': 8 * len(CONT), 'cat_cont': 4 * len(CAT) + 8 * len(CONT)}[family] * n * passes
    numpy_total = [x + y for x, y in zip(T['numpy_prepare'], T['numpy_pairs'])]
    report[mode] = {
        'Type': Type, 'pairs': len(pairs), 'pairs_on_device': len(off), 'max_abs_difference_to_numpy': err,
        'host_factorise_upload_ms': stat(T['host']), 'kernels_ms': stat(T['kernel']), 'columns_read_once_bound_ms': col_bytes / HBM * 1e3,
        'copy_back_frame_ms': stat(T['back']), 'total_ms': stat(T['total']),
        'numpy_factorise_ms': stat(T['numpy_prepare']), 'numpy_pairs_ms': stat(T['numpy_pairs']), 'numpy_total_ms': stat(numpy_total),
        'per_pair_pandas_sample_ms': t_pandas, 'per_pair_pandas_sample_pairs': ['%s x %s' % p for p in sample],
        'per_pair_pandas_EXTRAPOLATED_to_%d_pairs_ms' % len(off): t_pandas * len(off) / max(len(sample), 1)}
    print(mode, json.dumps(report[mode]), flush=True)
print(json.dumps(report))
