"""The two slow feature-engineering cells of the Rossmann notebook at their shape: `--stores` x `--days` rows (1115 x 942, about 1.05 M),
three event columns through get_TimeBeforeAfter and three numeric columns through get_RollingStats('8D', ['Sum']), per store.

Reported separately, per call of each function (medians over `--rounds` alternations with the baseline, after one warm-up of everything):
  host_ms    the host's factorise + np.lexsort by (group, time) + the uploads          (host clock around a device synchronise)
  kernel_ms  the HIP kernels (nnl_seg_event_gaps; nnl_seg_event_gaps + 2 x nnl_seg_rolling), HIP events on the stream, next to their
             traffic bound: the bytes the computation must read and write over the 6.29 TB/s copy rate
  back_ms    the copy back + the construction of the returned frame
  total_ms   the public call, end to end
Baselines, written here: `vectorised` = the same results from numpy / pandas without a Python loop over rows (np.maximum.accumulate
over the sorted rows; groupby().rolling('8D').sum() in both directions), checked against ours before anything is timed; `row_loop` = a
per-row .iloc loop per store and direction, which is how the notebook's own cell computes the gaps, timed on 1 % of the stores and
EXTRAPOLATED to all of them (labelled so in the output).
Usage: python tools/bench_tabular_features.py [--stores 1115] [--days 942] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralnetworklibrary_amd import ops  # noqa: E402
from neuralnetworklibrary_amd.Applications import StructuredData as SD  # noqa: E402
from neuralnetworklibrary_amd.General.Core import set_default_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--stores', type=int, default=1115)
ap.add_argument('--days', type=int, default=942)
ap.add_argument('--rounds', type=int, default=3)
a = ap.parse_args()
assert torch.cuda.is_available(), 'this is a GPU measurement'
set_default_device('cuda')
HBM = 6.29e12
EVENTS, COLS, DAY = ['Promo', 'StateHoliday', 'SchoolHoliday'], ['Sales', 'Customers', 'Open'], np.timedelta64(1, 'D')
SPAN = pd.Timedelta('8D').value

rs = np.random.RandomState(0)
n = a.stores * a.days
df = pd.DataFrame({'Store': np.repeat(np.arange(1, a.stores + 1), a.days),
                   'Date': np.tile(pd.date_range('2013-01-01', periods=a.days), a.stores)})
for ev, p in zip(EVENTS, (0.38, 0.03, 0.18)):
    df[ev] = (rs.random_sample(n) < p).astype('int64')
df['Sales'], df['Customers'], df['Open'] = rs.poisson(5700, n).astype('float64'), rs.poisson(630, n).astype('float64'), (rs.random_sample(n) < 0.83).astype('float64')
df = df.iloc[rs.permutation(n)].reset_index(drop=True)


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


def tba_phases(ev):
    "get_TimeBeforeAfter(df, ev, 'Date', 'Store', timescale=DAY) phase by phase, through the same helpers"
    def host():
        order, t, head, _ = SD._sorted_rows(df, 'Date', 'Store')
        event = (df[ev].to_numpy()[order] == 1).astype('uint8')
        return order, [SD._to_device(v) for v in (t, head, event)]
    h, (order, dev) = clock(host)
    k, res = device_ms(lambda: ops.seg_event_gaps(*dev, timescale=float(pd.Timedelta(DAY).value)))

    def back():
        gaps = torch.stack(res[:2]).cpu().numpy()
        out = df[['Date', 'Store']].iloc[order].copy()
        out[ev + 'Before'], out[ev + 'After'] = gaps[0], gaps[1]
        return out
    b, _ = clock(back)
    return h, k, b


def roll_phases():
    "get_RollingStats(df, COLS, '8D', ['Sum'], 'Date', 'Store') phase by phase"
    def host():
        order, t, head, _ = SD._sorted_rows(df, 'Date', 'Store')
        x = np.stack([df[c].to_numpy(dtype='float64')[order] for c in COLS])
        return order, [SD._to_device(v) for v in (t, head, x)]
    h, (order, (td, hd, xd)) = clock(host)

    def kernels():
        _, _, s, e = ops.seg_event_gaps(td, hd, torch.zeros(n, dtype=torch.uint8, device=td.device))
        return torch.stack([ops.seg_rolling(td, s, e, xd, ['Sum'], span=SPAN, forward=f) for f in (False, True)])
    k, both = device_ms(kernels)

    def back():
        v = both.cpu().numpy()
        out = pd.DataFrame({c + tag + 'Sum': v[d, 0, j] for d, tag in enumerate(('RollBwd', 'RollFwd')) for j, c in enumerate(COLS)},
                           index=pd.Index(df['Date'].to_numpy()[order], name='Date'))
        out['Store'] = df['Store'].to_numpy()[order]
        out['index'] = out.index
        return out
    b, _ = clock(back)
    return h, k, b


def vectorised_tba(ev):
    s = df[['Date', 'Store', ev]].sort_values(['Store', 'Date'], kind='stable')
    t, g, e = s['Date'].to_numpy().view('int64'), s['Store'].to_numpy(), s[ev].to_numpy() == 1
    idx = np.arange(len(s))
    first = np.maximum.accumulate(np.where(np.r_[True, g[1:] != g[:-1]], idx, -1))
    last = np.minimum.accumulate(np.where(np.r_[g[1:] != g[:-1], True], idx, len(s))[::-1])[::-1]
    prev = np.r_[-1, np.maximum.accumulate(np.where(e, idx, -1))[:-1]]
    nxt = np.r_[np.minimum.accumulate(np.where(e, idx, len(s))[::-1])[::-1][1:], len(s)]
    unit = float(pd.Timedelta(DAY).value)
    s[ev + 'Before'] = np.where(prev >= first, (t - t[np.maximum(prev, 0)]) / unit, np.nan)
    s[ev + 'After'] = np.where(nxt <= last, (t[np.minimum(nxt, len(s) - 1)] - t) / unit, np.nan)
    return s.drop(columns=[ev])


def vectorised_roll():
    s = df[['Date', 'Store'] + COLS].sort_values(['Store', 'Date'], kind='stable')
    bwd = s.groupby('Store').rolling('8D', on='Date', min_periods=1)[COLS].sum()
    r = s.iloc[::-1].copy()
    r['Date'] = pd.Timestamp('2000-01-01') + (s['Date'].max() - r['Date'])
    fwd = r.groupby('Store', sort=False).rolling('8D', on='Date', min_periods=1)[COLS].sum()
    return bwd[COLS].to_numpy(), fwd[COLS].to_numpy()[::-1]


def row_loop_tba(sub, ev):
    "gaps with a per-row .iloc loop per store and direction"
    out = []
    for _, X in sub.groupby('Store'):
        X = X.sort_values('Date')
        for step in (1, -1):
            Y, vals, last = X.iloc[::step], [], None
            for i in range(len(Y)):
                vals.append(np.nan if last is None else abs(Y['Date'].iloc[i] - last) / DAY)
                if Y[ev].iloc[i] == 1:
                    last = Y['Date'].iloc[i]
            out.append(vals)
    return out


# ---- correctness, which also warms everything up ---------------------------------------------------------------------------
ours = SD.get_TimeBeforeAfter(df, EVENTS[0], index_col='Date', groupby_col='Store', timescale=DAY)
want = vectorised_tba(EVENTS[0])
for c in (EVENTS[0] + 'Before', EVENTS[0] + 'After'):
    x, y = ours[c].to_numpy(), want[c].to_numpy()
    assert np.array_equal(ours.index, want.index) and ((x == y) | (np.isnan(x) & np.isnan(y))).all(), c
roll = SD.get_RollingStats(df, COLS, '8D', ['Sum'], index_col='Date', groupby_col='Store')
wb, wf = vectorised_roll()
assert np.array_equal(roll[[c + 'RollBwdSum' for c in COLS]].to_numpy(), wb)          # integer-valued columns: exact
assert np.array_equal(roll[[c + 'RollFwdSum' for c in COLS]].to_numpy(), wf)
tba_phases(EVENTS[0]); roll_phases()

sample = np.arange(1, max(a.stores // 100, 1) + 1)
sub = df[df['Store'].isin(sample)]
T = {k: [] for k in ('tba_host', 'tba_kernel', 'tba_back', 'tba_total', 'tba_vectorised', 'roll_host', 'roll_kernel', 'roll_back',
                     'roll_total', 'roll_vectorised', 'tba_row_loop_sample')}
for _ in range(a.rounds):
    for ev in EVENTS:
        T['tba_vectorised'].append(clock(lambda: vectorised_tba(ev))[0])
        T['tba_total'].append(clock(lambda: SD.get_TimeBeforeAfter(df, ev, index_col='Date', groupby_col='Store', timescale=DAY))[0])
        h, k, b = tba_phases(ev)
        T['tba_host'].append(h); T['tba_kernel'].append(k); T['tba_back'].append(b)
    T['roll_vectorised'].append(clock(vectorised_roll)[0])
    T['roll_total'].append(clock(lambda: SD.get_RollingStats(df, COLS, '8D', ['Sum'], index_col='Date', groupby_col='Store'))[0])
    h, k, b = roll_phases()
    T['roll_host'].append(h); T['roll_kernel'].append(k); T['roll_back'].append(b)
T['tba_row_loop_sample'].append(clock(lambda: row_loop_tba(sub, EVENTS[0]))[0])

C = len(COLS)
tba_bytes = n * (8 + 1 + 1 + 8 + 8 + 4 + 4)                      # t, head, event read; before, after, seg_start, seg_end written
roll_bytes = tba_bytes + 2 * n * (8 + 4 + 4 + 8 * C + 8 * C)     # + per direction: t, the two bounds and x read, one statistic written
stat = lambda v: {'median': float(np.median(v)), 'spread': float(max(v) - min(v))}
print(json.dumps({
    'rows': n, 'stores': a.stores, 'days': a.days, 'rounds': a.rounds,
    'get_TimeBeforeAfter_per_event_column_ms': {
        'host_sort_upload': stat(T['tba_host']), 'kernels': stat(T['tba_kernel']), 'kernels_traffic_bound_ms': tba_bytes / HBM * 1e3,
        'copy_back_frame': stat(T['tba_back']), 'total': stat(T['tba_total']), 'vectorised_numpy': stat(T['tba_vectorised']),
        'row_loop_extrapolated_from_%d_stores' % len(sample): T['tba_row_loop_sample'][0] * a.stores / len(sample)},
    'get_RollingStats_3_columns_8D_Sum_ms': {
        'host_sort_upload': stat(T['roll_host']), 'kernels': stat(T['roll_kernel']), 'kernels_traffic_bound_ms': roll_bytes / HBM * 1e3,
        'copy_back_frame': stat(T['roll_back']), 'total': stat(T['roll_total']), 'vectorised_pandas': stat(T['roll_vectorised'])},
    'results_equal': True}))
