"""Tabular data side: add_datepart, get_TimeBeforeAfter, get_RollingStats, ProcessDataFrame and StructuredDataObj.from_dataframes against
G21 (tests/golden/g21_tabular_features.npz: the real reference on the frames tools/gen_golden_tabular_features.py builds), and the two
HIP entries behind them (nnl_seg_event_gaps, nnl_seg_rolling, K12) over their scan-tile boundaries.

Tolerances.  Event gaps: an int64 difference divided once has nothing to round differently: exact.  Rolling Min / Max / Count, and Sum of
an integer-valued column: exact.  Rolling Sum / Mean against the np.longdouble restatement: the kernel adds the w entries of a window one
after another in fp64, so it is within w 2^-52 sum|x| of the exact value (w - 1 roundings of at most 2^-53 sum|x| each, the division and
the rounding of the restatement itself).  Std against the restatement: rtol 1e-12 (two passes in fp64 over at most ~1000 well-scaled
values).  Against the reference: the distance the generator recorded between the reference and the restatement (d_Sum, d_Mean, d_Std)
plus the kernel's own bound.  ProcessDataFrame: codes, targets and labels exact; continuous values and scaling values rtol 4 2^-23
(fp32 statistics a few ulp apart)."""
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import ROOT, load_golden
from tools.gen_golden_tabular_features import (CAT_VARS, CAT_VARS2, CONT_VARS, CONT_VARS2, DATEPART, DAY, ROLL_COLS, STATS, exact_like,
                                               frame_a, frame_b, process_frames, rolling_exact, seen_rows)

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import NnlError, lib
from neuralnetworklibrary_amd.Applications import StructuredData as SD

DEV = 'cuda'
EPS = 2.0 ** -52
RTOL32 = 4 * 2.0 ** -23
STD_RTOL = 1e-12


@pytest.fixture(scope='module')
def g21():
    return load_golden('g21_tabular_features')


def _gpu():
    from neuralnetworklibrary_amd.General.Core import set_default_device
    set_default_device(DEV)


def same(a, b):
    "equal values, NaN positions counting as equal"
    a, b = np.asarray(a, dtype='float64'), np.asarray(b, dtype='float64')
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ---- host side (no GPU) --------------------------------------------------------------------------------------------------

def test_generator_frames_are_the_ones_g21_was_made_from(g21):
    A, B = frame_a(), frame_b()
    assert np.array_equal(g21['a.in.index'], A.index) and np.array_equal(g21['b.in.index'], B.index)
    assert np.array_equal(g21['a.in.col.Date'], A['Date'].to_numpy().astype('datetime64[ns]').view('int64'))
    for c in ('Store', 'Promo', 'Holiday', 'x', 'k'):
        assert same(g21['a.in.col.' + c], A[c])
    for c in ('E', 'x', 'k'):
        assert same(g21['b.in.col.' + c], B[c])


def _labels(g21, prefix):
    return [dict(zip(g21['%s.%d.keys' % (prefix, j)].tolist(), g21['%s.%d.values' % (prefix, j)].tolist()))
            for j in range(int(g21[prefix + '.n']))]


def _check_processed(g21, prefix, xcat, xcont, y):
    assert np.array_equal(np.asarray(xcat), g21[prefix + '.xcat']) and np.asarray(xcat).dtype == np.int64
    xc = np.asarray(xcont)
    assert xc.dtype == np.float32
    np.testing.assert_allclose(xc, g21[prefix + '.xcont'], rtol=RTOL32, atol=0)
    if prefix + '.y' in g21:
        assert np.array_equal(np.asarray(y), g21[prefix + '.y']) and np.asarray(y).dtype == g21[prefix + '.y'].dtype
    else:
        assert y is None


def _process_case(tag):
    train, val, test = process_frames()
    if tag == 'c':
        return CAT_VARS, CONT_VARS, 'target', True, (train, val, test)
    return CAT_VARS2, CONT_VARS2, 'label', False, (train, seen_rows(val, train), seen_rows(test, train))


@pytest.mark.parametrize('tag', ['c', 'c2'])
def test_process_dataframe_matches_the_reference(g21, tag):
    cat_vars, cont_vars, target, unknown, frames = _process_case(tag)
    tr, va, te = frames
    assert [len(f) for f in frames] == g21[tag + '.rows'].tolist()
    copies = [f.copy() for f in frames]
    xcat, xcont, y, scaling, labels = SD.ProcessDataFrame(tr, cat_vars, cont_vars, target, 'by_df', 'median', None, unknown)
    _check_processed(g21, tag + '.train', xcat, xcont, y)
    assert xcat.index.equals(tr.index) and list(xcat.columns) == [v for v in cat_vars if v != target]
    want = _labels(g21, tag + '.labels')
    assert labels == want and [list(d) for d in labels] == [list(d) for d in want]          # the same keys in the same order
    assert list(scaling) == g21[tag + '.scaling.vars'].tolist()
    np.testing.assert_allclose(np.array([[float(m), float(s)] for m, s in scaling.values()]), g21[tag + '.scaling'], rtol=RTOL32, atol=0)
    res = SD.ProcessDataFrame(va, cat_vars, cont_vars, target, scaling, 'median', labels, unknown)
    _check_processed(g21, tag + '.val', *res[:3])
    assert res[3] is scaling and res[4] is labels
    xcat_vars, xcont_vars = [v for v in cat_vars if v != target], [v for v in cont_vars if v != target]
    res = SD.ProcessDataFrame(te, xcat_vars, xcont_vars, None, scaling, 'median', labels, unknown)
    _check_processed(g21, tag + '.test', *res[:3])
    for f, c in zip(frames, copies):
        assert f.equals(c) and list(f.dtypes) == list(c.dtypes), 'ProcessDataFrame modified its input frame'


def test_process_dataframe_missing_none_fill_and_unscaled():
    "None counts as missing like NaN; fill_missing 'mean' / a constant; scale_cont='No' returns no scaling values"
    df = pd.DataFrame({'c': ['b', None, 'a', np.nan, 'b'], 'v': [1.0, np.nan, 3.0, 5.0, np.nan], 'y': [0.0, 1.0, 2.0, 3.0, 4.0]})
    xcat, xcont, y, scaling, labels = SD.ProcessDataFrame(df, ['c'], ['v', 'y'], 'y', 'No', 'mean')
    assert labels == [{'a': 1, 'b': 2, 'unknown': 0}] and xcat['c'].tolist() == [2, 0, 1, 0, 2] and scaling is None
    assert xcont['v'].tolist() == [1.0, 3.0, 3.0, 5.0, 3.0] and y.dtype == np.float32
    xcont = SD.ProcessDataFrame(df, ['c'], ['v', 'y'], 'y', 'No', -1)[1]
    assert xcont['v'].tolist() == [1.0, -1.0, 3.0, 5.0, -1.0]


@pytest.mark.parametrize('tag', ['c', 'c2'])
def test_from_dataframes_chains_the_three_frames(g21, tag):
    cat_vars, cont_vars, target, unknown, frames = _process_case(tag)
    copies = [f.copy() for f in frames]
    data = SD.StructuredDataObj.from_dataframes(frames[0], frames[1], cat_vars, cont_vars, target, bs=8, unknown_category=unknown,
                                                num_workers=0, test_df=frames[2])
    assert data.target_type == ('cont' if tag == 'c' else 'cat') and data.bs == 8
    for name, ds in (('train', data.train_ds), ('val', data.val_ds), ('test', data.test_ds)):
        _check_processed(g21, '%s.%s' % (tag, name), ds.x_cat, ds.x_cont, ds.y if name != 'test' else None)
        assert (ds.n_cat, ds.n_cont) == (2, 2)
    assert data.category_labels == _labels(g21, tag + '.labels')
    np.testing.assert_allclose(np.array([[float(m), float(s)] for m, s in data.scaling_values.values()]), g21[tag + '.scaling'],
                               rtol=RTOL32, atol=0)
    assert np.array_equal(data.test_ds.y, np.zeros(len(frames[2]), dtype='float32'))
    for f, c in zip(frames, copies):
        assert f.equals(c)
    unscaled = SD.StructuredDataObj.from_dataframes(frames[0], frames[1], cat_vars, cont_vars, target, bs=8, scale_cont=False,
                                                    unknown_category=unknown, num_workers=0)
    assert unscaled.scaling_values is None and unscaled.test_ds is None
    filled = frames[0][['a', 'b']].astype('float32')
    assert np.array_equal(unscaled.train_ds.x_cont, filled.fillna(filled.median()).to_numpy())


def test_add_datepart_matches_pandas_fields(g21):
    A = frame_a()
    before = A.copy()
    assert SD.add_datepart(A, 'Date') is None                  # in place
    assert list(A.columns) == list(before.columns) + DATEPART
    for name in DATEPART[:-1]:
        assert pd.api.types.is_integer_dtype(A[name]), name
        assert np.array_equal(A[name].to_numpy(), g21['d.' + name]), name
    assert A['days_elapsed'].dtype == np.float64 and np.array_equal(A['days_elapsed'].to_numpy(), g21['d.days_elapsed'])
    assert A[list(before.columns)].equals(before)
    B = before.copy()
    B['Date'] = B['Date'].dt.strftime('%Y-%m-%d')              # strings are parsed, `start` is honoured
    SD.add_datepart(B, 'Date', start='2014-12-25')
    assert np.array_equal(B['days_elapsed'].to_numpy(), g21['d.days_elapsed_from_2014'])
    assert np.array_equal(B['week'].to_numpy(), g21['d.week'])


def test_abi_entries_validate_before_any_hip_call():
    "both entries return -1 and name themselves: no GPU is needed, so no HIP call was made"
    one = torch.zeros(8, dtype=torch.int64)
    p = one.data_ptr()
    for n in (0, -3, 2 ** 31):
        assert lib.nnl_seg_event_gaps(p, p, p, n, 1.0, p, p, p, p, None) == -1
        assert b'seg_event_gaps' in lib.nnl_last_error()
        assert lib.nnl_seg_rolling(p, p, p, p, n, 1, 3, 0, 0, 1, p, None) == -1
        assert b'seg_rolling' in lib.nnl_last_error()
    for k in range(7):
        args = [p] * 3 + [1, 1.0] + [p] * 4
        args[k if k < 3 else k + 2] = None
        assert lib.nnl_seg_event_gaps(*args, None) == -1
        assert b'seg_event_gaps' in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
    for k in (0, 1, 2, 3, 10):
        args = [p] * 4 + [1, 1, 3, 0, 0, 1, p]
        args[k] = None
        assert lib.nnl_seg_rolling(*args, None) == -1
        assert b'seg_rolling' in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
    for count_window, span in ((3, 4), (0, 0), (-1, 5)):
        assert lib.nnl_seg_rolling(p, p, p, p, 1, 1, count_window, span, 0, 1, p, None) == -1
        assert b'seg_rolling' in lib.nnl_last_error() and b'count_window' in lib.nnl_last_error()
    assert lib.nnl_seg_rolling(p, p, p, p, 1, 1, 3, 0, 0, 0, p, None) == -1 and b'stat_mask' in lib.nnl_last_error()
    assert lib.nnl_seg_rolling(p, p, p, p, 1, 1, 3, 0, 0, 64, p, None) == -1 and b'stat_mask' in lib.nnl_last_error()
    assert lib.nnl_seg_event_gaps(p, p, p, 1, 0.0, p, p, p, p, None) == -1 and b'timescale' in lib.nnl_last_error()


def test_ops_refuse_cpu_tensors_and_export_the_tile():
    t, h = torch.arange(4), torch.ones(4, dtype=torch.uint8)
    with pytest.raises(NnlError):
        ops.seg_event_gaps(t, h, h)
    s = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(NnlError):
        ops.seg_rolling(t, s, s, torch.zeros(1, 4, dtype=torch.float64), ['Sum'], count_window=2)
    header = open(os.path.join(ROOT, 'include', 'nnl.h')).read()
    assert int(re.search(r'#define\s+NNL_SEG_SCAN_TILE\s+(\d+)', header).group(1)) == ops.SEG_SCAN_TILE
    assert ops.ROLL_STATS == STATS
    for st in ('seg_event_gaps', 'seg_rolling', 'SEG_SCAN_TILE'):
        assert st in ops.__all__
    for name in ('add_datepart', 'get_TimeBeforeAfter', 'get_RollingStats', 'ProcessDataFrame'):
        ns = {}
        exec('from neuralnetworklibrary_amd.Applications.StructuredData import *', ns)
        assert name in ns


def test_duplicate_or_missing_times_raise_before_any_upload():
    "ValueError on the host: this runs without a GPU, where an upload or a kernel call would raise NnlError instead"
    A = frame_a()
    dup = pd.concat([A, A.iloc[[5]]])
    with pytest.raises(ValueError, match='duplicate'):
        SD.get_TimeBeforeAfter(dup, 'Promo', index_col='Date', groupby_col='Store', timescale=DAY)
    with pytest.raises(ValueError, match='duplicate'):
        SD.get_RollingStats(dup, ROLL_COLS, '8D', ['Sum'], index_col='Date', groupby_col='Store')
    B = frame_b()
    dupb = pd.concat([B, B.iloc[[0]]])
    with pytest.raises(ValueError, match='duplicate'):
        SD.get_TimeBeforeAfter(dupb, 'E')
    with pytest.raises(ValueError, match='duplicate'):
        SD.get_RollingStats(dupb, ROLL_COLS, 3, STATS)
    nat = A.copy()
    nat.loc[nat.index[3], 'Date'] = pd.NaT
    with pytest.raises(ValueError, match='NaT'):
        SD.get_TimeBeforeAfter(nat, 'Promo', index_col='Date', groupby_col='Store', timescale=DAY)
    with pytest.raises(ValueError, match='NaT'):
        SD.get_RollingStats(nat, ROLL_COLS, '8D', ['Sum'], index_col='Date', groupby_col='Store')
    nanidx = B.copy()
    nanidx.index = [np.nan] + list(B.index[1:])
    with pytest.raises(ValueError, match='NaN'):
        SD.get_TimeBeforeAfter(nanidx, 'E')
    with pytest.raises(ValueError, match='datetime'):
        SD.get_RollingStats(B, ROLL_COLS, '8D', ['Sum'])          # a time window on an integer index
    # the same day in DIFFERENT stores is no duplicate
    order, t, head, is_dt = SD._sorted_rows(A.assign(Date=A['Date'].iloc[0], Store=np.arange(len(A))), 'Date', 'Store')
    assert head.all() and is_dt and np.array_equal(order, np.arange(len(A)))


def test_host_sort_is_the_lexsort_by_group_then_time():
    "groups in sorted label order, time ascending inside a group, rows without a group label dropped (as groupby drops them)"
    A = frame_a()
    codes = pd.factorize(A['Store'], sort=True)[0]
    t = A['Date'].to_numpy().astype('datetime64[ns]').view('int64')
    order, ts, head, is_dt = SD._sorted_rows(A, 'Date', 'Store')
    assert is_dt and np.array_equal(order, np.lexsort((t, codes))) and np.array_equal(ts, t[order]) and head.dtype == np.uint8
    assert np.array_equal(np.flatnonzero(head), [0, 2, 132, 133])                   # stores 3, 7, 11, 20: 2, 130, 1 and 70 rows
    labelled = A['Store'].astype(object).where(A['Store'] != 7, None)               # store 7 loses its label
    order2, _, head2, _ = SD._sorted_rows(A.assign(Store=labelled), 'Date', 'Store')
    assert np.array_equal(order2, order[(A['Store'].to_numpy() != 7)[order]]) and head2.sum() == 3
    B = frame_b()
    order, ts, head, is_dt = SD._sorted_rows(B, None, None)
    assert not is_dt and np.array_equal(ts, np.sort(B.index)) and head.tolist() == [1] + [0] * 69
    with pytest.raises(ValueError, match='group label'):
        SD._sorted_rows(A.assign(Store=np.nan), 'Date', 'Store')


# ---- the frames on the GPU, against G21 ------------------------------------------------------------------------------------

def _frame_matches(g21, prefix, got, float_cols):
    assert list(got.columns) == g21[prefix + '.columns'].tolist()
    assert np.array_equal(np.asarray(got.index), g21[prefix + '.index'])
    for c in got.columns:
        want = g21['%s.col.%s' % (prefix, c)]
        v = got[c]
        if pd.api.types.is_datetime64_any_dtype(v):
            assert np.array_equal(v.to_numpy().astype('datetime64[ns]').view('int64'), want), c
        elif c in float_cols:
            assert v.dtype == np.float64 and same(v.to_numpy(), want), c           # exact, NaN positions included
            assert np.isnan(want).any() and (~np.isnan(want)).any()
        else:
            assert np.array_equal(v.to_numpy(), want), c


@pytest.mark.gpu
@pytest.mark.parametrize('event', ['Promo', 'Holiday'])
def test_time_before_after_frame_a_equals_the_reference(g21, event):
    _gpu()
    A = frame_a()
    before = A.copy()
    got = SD.get_TimeBeforeAfter(A, event, index_col='Date', groupby_col='Store', timescale=DAY)
    _frame_matches(g21, 'a.tba.' + event, got, [event + 'Before', event + 'After'])
    assert A.equals(before) and list(A.columns) == list(before.columns)
    again = SD.get_TimeBeforeAfter(A, event, index_col='Date', groupby_col='Store', timescale=pd.Timedelta(days=1))
    assert again.equals(got)


@pytest.mark.gpu
def test_time_before_after_frame_b_equals_the_reference(g21):
    _gpu()
    B = frame_b()
    before = B.copy()
    got = SD.get_TimeBeforeAfter(B, 'E', timescale=1)
    _frame_matches(g21, 'b.tba.E', got, ['EBefore', 'EAfter'])
    assert B.equals(before) and 'index' not in B.columns
    kept = SD.get_TimeBeforeAfter(B, 'E', keep_cols=['k'], timescale=2)
    assert list(kept.columns) == ['index', 'k', 'EBefore', 'EAfter'] and same(kept['EBefore'], g21['b.tba.E.col.EBefore'] / 2)
    assert np.array_equal(kept['k'].to_numpy(), B.loc[kept.index, 'k'].to_numpy())


def _check_rolling_frame(g21, tag, got, exact, counts, abssum):
    """got: our frame; exact / counts / abssum: {column name: [rows]} from the np.longdouble restatement (recomputed here, and equal to
    what G21 stores), the window's number of entries and its sum |x|"""
    assert list(got.columns) == g21[tag + '.roll.columns'].tolist()
    assert np.array_equal(np.asarray(got.index.view('int64') if isinstance(got.index, pd.DatetimeIndex) else got.index), g21[tag + '.roll.index'])
    for name, ex in exact.items():
        assert same(ex, g21['%s.roll.%s_exact' % (tag, name)]), name
        st = [s for s in STATS if name.endswith(s)][0]
        ref, v = g21['%s.roll.%s' % (tag, name)], got[name].to_numpy()
        assert v.dtype == np.float64 and np.array_equal(np.isnan(v), np.isnan(ex)) and np.array_equal(np.isnan(v), np.isnan(ref)), name
        base = name[:-len(st)]
        ok = ~np.isnan(ex)
        if st in ('Min', 'Max', 'Count') or (st == 'Sum' and name.startswith('k')):
            assert same(v, ref) and same(v, ex), name                                  # bit-equal
            continue
        own = STD_RTOL * np.abs(ex) if st == 'Std' else counts[base] * EPS * abssum[base]
        err_exact, err_ref = np.abs(v - ex)[ok], np.abs(v - ref)[ok]
        print('%s %s: max |ours - exact| %.3e (bound %.3e), max |ours - reference| %.3e (recorded d %.3e)'
              % (tag, name, err_exact.max(), own[ok].max(), err_ref.max(), float(g21['%s.roll.d_%s' % (tag, st)])))
        assert (err_exact <= own[ok]).all(), name
        assert (err_ref <= float(g21['%s.roll.d_%s' % (tag, st)]) + own[ok]).all(), name


def _exact_for(ref_cols, t, groups, values, window):
    "the restatement laid out like the frame, plus per (column, direction) the number of window entries and the window's sum |x|"
    frame = pd.DataFrame({c: np.zeros(len(t)) for c in ref_cols if 'Roll' in c})
    exact = exact_like(frame, t, groups, values, window)
    counts, abssum = {}, {}
    for col in ROLL_COLS:
        for tag in ('RollBwd', 'RollFwd'):
            counts[col + tag] = exact[col + tag + 'Count']
            abssum[col + tag] = exact_like(frame, t, groups, {c: np.abs(values[c]) for c in values}, window)[col + tag + 'Sum']
    return exact, counts, abssum


@pytest.mark.gpu
def test_rolling_stats_frame_a_time_window(g21):
    _gpu()
    A = frame_a()
    before = A.copy()
    got = SD.get_RollingStats(A, ROLL_COLS, '8D', STATS, index_col='Date', groupby_col='Store')
    assert A.equals(before)
    assert np.array_equal(got['Store'].to_numpy(), g21['a.roll.Store'])
    assert np.array_equal(got['index'].to_numpy().astype('datetime64[ns]').view('int64'), g21['a.roll.index_col'])
    assert got.index.name == 'Date'
    S = A.set_index(['Store', 'Date'])
    values = {c: S.loc[list(zip(got['Store'], got.index)), c].to_numpy() for c in ROLL_COLS}
    exact, counts, abssum = _exact_for(got.columns, got.index.view('int64'), got['Store'].to_numpy(), values, ('span', 8 * 86400 * 10 ** 9))
    _check_rolling_frame(g21, 'a', got, exact, counts, abssum)
    only_sum = SD.get_RollingStats(A, ['k'], pd.Timedelta(days=8), ['Sum'], index_col='Date', groupby_col='Store')
    assert list(only_sum.columns) == ['kRollBwdSum', 'kRollFwdSum', 'Store', 'index']
    assert same(only_sum['kRollFwdSum'], got['kRollFwdSum']) and same(only_sum['kRollBwdSum'], got['kRollBwdSum'])


@pytest.mark.gpu
def test_rolling_stats_frame_b_count_window(g21):
    _gpu()
    B = frame_b()
    before = B.copy()
    got = SD.get_RollingStats(B, ROLL_COLS, 3, STATS)
    assert B.equals(before)
    t = np.asarray(got.index, dtype='int64')
    values = {c: B.loc[got.index, c].to_numpy() for c in ROLL_COLS}
    exact, counts, abssum = _exact_for(got.columns, t, np.zeros(len(t), dtype='int64'), values, 3)
    _check_rolling_frame(g21, 'b', got, exact, counts, abssum)


# ---- the two entries over the scan's tile boundaries -------------------------------------------------------------------------

def gaps_by_definition(t, head, event, timescale):
    "the reference's loop (StructuredData.py:496-515), one group after the other: append first, then update last_event"
    n = len(t)
    before, after = np.full(n, np.nan), np.full(n, np.nan)
    seg_start, seg_end = np.zeros(n, dtype='int32'), np.zeros(n, dtype='int32')
    starts = [i for i in range(n) if i == 0 or head[i]]
    for a, b in zip(starts, starts[1:] + [n]):
        seg_start[a:b], seg_end[a:b] = a, b - 1
        last = None
        for i in range(a, b):
            if last is not None:
                before[i] = float(int(t[i]) - int(t[last])) / timescale
            if event[i] == 1:
                last = i
        last = None
        for i in range(b - 1, a - 1, -1):
            if last is not None:
                after[i] = float(int(t[last]) - int(t[i])) / timescale
            if event[i] == 1:
                last = i
    return before, after, seg_start, seg_end


def _layouts():
    "name -> (t, head, event): the group boundaries and events sit where the three-launch scan hands over between tiles"
    T = ops.SEG_SCAN_TILE
    rs = np.random.RandomState(2104)
    out = {}
    n = 2 * T + 37

    def times(n):
        return np.cumsum(rs.randint(1, 9, n)).astype('int64') * 1000 + 5

    head = np.zeros(n, dtype='uint8'); head[0] = 1
    event = np.zeros(n, dtype='uint8'); event[[3, T // 2]] = 1
    out['one_group_three_tiles_events_in_tile0'] = (times(n), head, event)            # the carry must cross two tiles
    event = np.zeros(n, dtype='uint8'); event[[2 * T + 1, 2 * T + 30]] = 1
    out['one_group_three_tiles_events_in_tile2'] = (times(n), head.copy(), event)     # the same for the backward scan
    head = np.zeros(n, dtype='uint8'); head[[0, T, 2 * T - 1]] = 1
    event = (rs.random_sample(n) < 0.1).astype('uint8'); event[[T - 1, T, 2 * T - 2, 2 * T - 1, 2 * T]] = 1
    out['heads_on_rows_T_and_2T_minus_1'] = (times(n), head, event)
    event = event.copy(); event[T - 40:T + 40] = 0; event[2 * T - 40:2 * T + 40] = 0
    out['heads_on_tile_edges_no_event_near_them'] = (times(n), head.copy(), event)
    out['300_groups_of_one_row'] = (times(300), np.ones(300, dtype='uint8'), (rs.random_sample(300) < 0.5).astype('uint8'))
    out['n_equals_1'] = (times(1), np.ones(1, dtype='uint8'), np.ones(1, dtype='uint8'))
    out['exactly_one_tile'] = (times(T), (rs.random_sample(T) < 0.02).astype('uint8'), (rs.random_sample(T) < 0.1).astype('uint8'))
    out['one_tile_and_one_row'] = (times(T + 1), (rs.random_sample(T + 1) < 0.02).astype('uint8'), (rs.random_sample(T + 1) < 0.1).astype('uint8'))
    return out


LAYOUTS = _layouts()


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_seg_event_gaps_across_tile_boundaries(name):
    t, head, event = LAYOUTS[name]
    want = gaps_by_definition(t, head, event, 3000.0)
    dev = [torch.from_numpy(a).to(DEV) for a in (t, head, event)]
    got = [a.cpu().numpy() for a in ops.seg_event_gaps(*dev, timescale=3000.0)]
    assert got[0].dtype == np.float64 and got[2].dtype == np.int32
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert same(got[0], want[0]) and same(got[1], want[1])
    if name == 'one_group_three_tiles_events_in_tile0':
        T = ops.SEG_SCAN_TILE
        assert got[0][-1] == float(t[-1] - t[T // 2]) / 3000.0 and np.isnan(got[1][T:]).all() and np.isnan(got[0][:4]).all()
    # the inputs are read only, and a second call gives the same bits (the carries pass through the outputs: nothing may linger)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(dev, (t, head, event)))
    again = [a.cpu().numpy() for a in ops.seg_event_gaps(*dev, timescale=3000.0)]
    assert all(same(a, b) for a, b in zip(got, again))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_seg_rolling_across_tile_boundaries(name):
    "a count window of T + 5 rows reaches across a tile; a span window of about 40 rows as well; against the np.longdouble restatement"
    T = ops.SEG_SCAN_TILE
    t, head, _ = LAYOUTS[name]
    n = len(t)
    rs = np.random.RandomState(2105)
    x = np.stack([rs.standard_normal(n), rs.randint(0, 50, n).astype('float64')])
    x[0, rs.random_sample(n) < 0.05] = np.nan
    _, _, seg_start, seg_end = gaps_by_definition(t, head, np.zeros(n, dtype='uint8'), 1.0)
    td, sd, ed, xd = [torch.from_numpy(a).to(DEV) for a in (t, seg_start, seg_end, x)]
    h0, h1, _, _ = ops.seg_event_gaps(td, torch.from_numpy(head).to(DEV), torch.zeros(n, dtype=torch.uint8, device=DEV))
    assert torch.isnan(h0).all() and torch.isnan(h1).all()
    for window, kw in ((T + 5, dict(count_window=T + 5)), (('span', 180000), dict(span=180000))):
        for fwd in (False, True):
            got = ops.seg_rolling(td, sd, ed, xd, STATS, forward=fwd, **kw).cpu().numpy()
            assert got.shape == (6, 2, n)
            for c in range(2):
                ex = {st: np.full(n, np.nan) for st in STATS + ['Abs']}
                for a in np.unique(seg_start):
                    rows = np.where(seg_start == a)[0]
                    e = rolling_exact(t[rows], x[c][rows], window, fwd)
                    e['Abs'] = rolling_exact(t[rows], np.abs(x[c][rows]), window, fwd)['Sum']
                    for st in ex:
                        ex[st][rows] = e[st]
                for s, st in enumerate(STATS):
                    v = got[s, c]
                    assert np.array_equal(np.isnan(v), np.isnan(ex[st])), (st, c, fwd)
                    ok = ~np.isnan(ex[st])
                    if st in ('Min', 'Max', 'Count') or (st == 'Sum' and c == 1):
                        assert same(v, ex[st]), (st, c, fwd)
                    elif st == 'Std':
                        assert (np.abs(v - ex[st])[ok] <= STD_RTOL * np.abs(ex[st])[ok]).all(), (st, c, fwd)
                    else:
                        assert (np.abs(v - ex[st])[ok] <= (ex['Count'] * EPS * ex['Abs'])[ok]).all(), (st, c, fwd)
            if not fwd and 'count_window' in kw:
                sub = ops.seg_rolling(td, sd, ed, xd, ['Count', 'Sum'], forward=fwd, **kw).cpu().numpy()      # a subset, in the caller's order
                assert same(sub[0], got[5]) and same(sub[1], got[0])


# ---- end to end ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_notebook_cell_sequence_from_dataframes_to_predict():
    "add_datepart -> get_TimeBeforeAfter -> get_RollingStats -> from_dataframes -> fit -> predict('test') on a synthetic Rossmann-like frame"
    from neuralnetworklibrary_amd.General.Learner import Learner
    _gpu()
    Learner.verbose = False
    rs = np.random.RandomState(2106)
    stores, days = 8, 40
    df = pd.DataFrame({'Store': np.repeat(np.arange(1, stores + 1), days),
                       'Date': np.tile(pd.date_range('2015-01-01', periods=days).strftime('%Y-%m-%d'), stores)})
    n = len(df)
    df['Promo'] = (rs.random_sample(n) < 0.2).astype('int64')
    df['StoreType'] = rs.choice(['a', 'b', 'c'], n)
    df['Customers'] = rs.poisson(30, n).astype('float64')
    df = df.iloc[rs.permutation(n)].reset_index(drop=True)
    SD.add_datepart(df, 'Date')
    tba = SD.get_TimeBeforeAfter(df, 'Promo', index_col='Date', groupby_col='Store', timescale=np.timedelta64(1, 'D'))
    roll = SD.get_RollingStats(df, ['Customers'], '8D', ['Sum'], index_col='Date', groupby_col='Store')
    df = df.merge(tba, on=['Store', 'Date']).merge(roll.reset_index(drop=True).rename(columns={'index': 'Date'}), on=['Store', 'Date'])
    assert len(df) == n and df['CustomersRollBwdSum'].notna().all()
    df['Sales'] = (df['Customers'] * 3 + df['Promo'] * 20 + rs.standard_normal(n)).astype('float32')
    cat_vars = ['Store', 'StoreType', 'dayofweek', 'Promo']
    cont_vars = ['PromoBefore', 'PromoAfter', 'CustomersRollBwdSum', 'CustomersRollFwdSum', 'days_elapsed', 'Sales']
    train_df, val_df, test_df = df[:200], df[200:256], df[256:].drop(columns=['Sales'])
    data = SD.StructuredDataObj.from_dataframes(train_df, val_df, cat_vars, cont_vars, 'Sales', bs=64, test_df=test_df,
                                                device_resident=True, seed=5)
    xcat, xcont, y, _, _ = SD.ProcessDataFrame(val_df, cat_vars, cont_vars, 'Sales', data.scaling_values, 'median', data.category_labels)
    assert not np.isnan(xcont.to_numpy()).any()
    (bcat, bcont), by = next(iter(data.val_dl))                 # the loaders' first minibatch = the rows of the processed arrays
    assert bcat.is_cuda and np.array_equal(bcat.cpu().numpy(), xcat.to_numpy()[:64])
    assert np.array_equal(bcont.cpu().numpy(), xcont.to_numpy()[:64]) and np.array_equal(by.cpu().numpy(), y[:64])
    assert np.array_equal(data.val_ds.x_cat, xcat.to_numpy()) and np.array_equal(data.val_ds.x_cont, xcont.to_numpy())
    torch.manual_seed(0)
    net = SD.StructuredDataNet.from_dataobj(data, [32, 1])
    learner = Learner('/tmp/nnl_test_tabular_features', data, net, optimizer='Adam')
    learner.fit(1e-2, 1)
    assert len(learner.loss_sched) == len(data.train_dl) and np.isfinite(learner.loss_sched).all()
    assert np.isfinite(learner.evaluate('val')[0])
    pred = learner.predict('test')
    assert pred.shape == (len(test_df),) and np.isfinite(pred).all()
