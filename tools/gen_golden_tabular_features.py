"""Golden vectors G21 for the tabular data side (reference Applications/StructuredData.py: add_datepart :432-458,
get_TimeBeforeAfter :460-519, get_RollingStats :530-607, ProcessDataFrame :614-801).

Runs the REAL reference on CPU through oracle/_ref_import.py (read-only) and writes arrays only (loadable with allow_pickle=False) to
tests/golden/g21_tabular_features.npz.  The input frames are built here from seeded np.random.RandomState draws and then shuffled;
the tests rebuild them with the same functions (`frame_a`, `frame_b`, `process_frames`) and G21 stores their columns as a cross-check.

  (a) frame A, 203 rows: stores 11, 3, 20 and 7 with 1, 2, 70 and 130 rows on distinct days out of 200.  Event column 'Promo': none in
      the one-row store, every row of the two-row store, about 20 % in the two large stores; event column 'Holiday' (added so that every
      placement has a group of its own): the one row of store 11 (every row an event), none in store 3, only the FIRST day of store 20,
      only the LAST day of store 7.  'x' ~ N(0, 1) with three NaNs, one of them the single row of store 11 (alone in its 8-day windows);
      'k' integer-valued.  get_TimeBeforeAfter(A, 'Promo' / 'Holiday', index_col='Date', groupby_col='Store',
      timescale=np.timedelta64(1, 'D')) and get_RollingStats(A, ['x', 'k'], '8D', all six statistics, index_col='Date',
      groupby_col='Store').
  (b) frame B: one group of 70 rows with a plain integer index (distinct values out of 150): get_TimeBeforeAfter(B, 'E', timescale=1)
      and get_RollingStats(B, ['x', 'k'], 3, all six statistics).
  (c) ProcessDataFrame on train (40 rows), then on val (15 rows) and test (12 rows, no target) with the returned labels and scaling:
      a string categorical column and a float-coded integer one (values >= 10, so the string sort matters), both with np.nan entries,
      two continuous columns with NaNs, a continuous target, val / test values unseen in train.  (c2): a categorical target and
      unknown_category=False; the reference then ASSUMES that no value is missing or unseen (:669-670: an unlabelled category stays a
      string and its astype('int64') raises, or, float-coded, becomes its own integer), so for (c2) the categorical INPUT columns of
      the same frames are restricted to what the reference defines: missing entries stay (they are the category 'nan' there) and the
      val / test rows that hold a value unseen in train are left out.
      Missing values are np.nan, not None: under the installed pandas the reference turns None into a category called 'None'.
  (d) add_datepart: the reference's own fails under the installed pandas (`.dt.week` is gone), so these expectations are pandas' own
      calendar fields, computed here field by field (week = .dt.isocalendar().week).

Rolling statistics: besides the reference's values the generator computes every statistic from its definition in np.longdouble
(two-pass Std) and stores them as `*_exact`, and the largest distance between the reference and that restatement per statistic as
`d_Sum`, `d_Mean`, `d_Std`.  It asserts bit equality for Min, Max and Count on all columns and for Sum on the integer-valued
column, and that d_Sum and d_Mean lie within L 2^-52 max|x| with L the longest group: a bound on pandas' add-and-remove accumulator,
which carries its error over a whole group and not only over one window.
Usage: python tools/gen_golden_tabular_features.py   (needs the reference checkout the oracle shim points at)"""
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g21_tabular_features.npz')
STATS = ['Sum', 'Min', 'Max', 'Mean', 'Std', 'Count']
ROLL_COLS = ['x', 'k']
DAY = np.timedelta64(1, 'D')
A_STORES, A_SIZES, A_DAYS = [11, 3, 20, 7], [1, 2, 70, 130], 200
DATEPART = ['week', 'month', 'year', 'dayofweek', 'dayofmonth', 'dayofyear', 'is_month_end', 'is_month_start', 'is_quarter_end',
            'is_quarter_start', 'is_year_end', 'is_year_start', 'days_elapsed']


def frame_a():
    "203 rows, shuffled: Store, Date, Promo, Holiday, x, k (see the module docstring)"
    rs = np.random.RandomState(2101)
    parts = []
    for store, size in zip(A_STORES, A_SIZES):
        days = np.sort(rs.choice(A_DAYS, size, replace=False))
        promo = (rs.random_sample(size) < 0.2).astype('int64')
        holiday = np.zeros(size, dtype='int64')
        if size == 1:
            promo[:], holiday[:] = 0, 1
        elif size == 2:
            promo[:] = 1
        elif size == 70:
            holiday[0] = 1
        else:
            holiday[-1] = 1
        parts.append(pd.DataFrame({'Store': store, 'Date': pd.Timestamp('2015-01-01') + pd.to_timedelta(days, unit='D'), 'Promo': promo,
                                   'Holiday': holiday, 'x': rs.standard_normal(size), 'k': rs.randint(0, 50, size).astype('float64')}))
    df = pd.concat(parts, ignore_index=True)
    nan_rows = [0, 1 + 2 + 17, 1 + 2 + 70 + 64]           # the one row of store 11, one row of store 20, one of store 7
    df.loc[nan_rows, 'x'] = np.nan
    df = df.iloc[rs.permutation(len(df))].reset_index(drop=True)
    df.index = df.index + 1000                            # an index that is not 0 .. n-1: it must survive unchanged
    return df


def frame_b():
    "one group of 70 rows on a shuffled plain integer index: E, x, k"
    rs = np.random.RandomState(2102)
    idx = rs.choice(150, 70, replace=False)
    df = pd.DataFrame({'E': (rs.random_sample(70) < 0.2).astype('int64'), 'x': rs.standard_normal(70),
                       'k': rs.randint(0, 50, 70).astype('float64')}, index=idx)
    df.loc[idx[5], 'x'] = np.nan
    return df


CAT_VARS, CONT_VARS = ['color', 'code'], ['a', 'b', 'target']
CAT_VARS2, CONT_VARS2 = ['color', 'code', 'label'], ['a', 'b']


def process_frames():
    "train (40), val (15) and test (12 rows) for ProcessDataFrame: color, code, a, b, target (continuous), label (categorical)"
    rs = np.random.RandomState(2103)

    def make(n, colors, codes, nan_every):
        df = pd.DataFrame({'color': rs.choice(colors, n).astype(object), 'code': rs.choice(codes, n).astype('float64'),
                           'a': rs.standard_normal(n) * 3 + 1, 'b': rs.random_sample(n) * 100, 'target': rs.standard_normal(n),
                           'label': rs.choice(['no', 'yes', 'maybe'], n).astype(object)})
        df.loc[::nan_every, 'color'] = np.nan
        df.loc[1::nan_every, 'code'] = np.nan
        df.loc[2::nan_every, 'a'] = np.nan
        df.loc[3::nan_every, 'b'] = np.nan
        return df.iloc[rs.permutation(n)].reset_index(drop=True)
    train = make(40, ['red', 'green', 'blue', 'Zinc'], [2, 7, 10, 11, 100, 23], 9)
    val = make(15, ['red', 'green', 'blue', 'Zinc', 'mauve'], [2, 7, 10, 11, 100, 23, 5, 110], 6)
    test = make(12, ['red', 'blue', 'teal'], [2, 10, 100, 9], 5).drop(columns=['target', 'label'])
    return train, val, test


def seen_rows(df, train):
    "rows of df whose categorical input values all occur in train (missing counts as a value): what (c2) keeps"
    ok = np.ones(len(df), dtype=bool)
    for var in ['color', 'code']:
        known = set(train[var].dropna())
        ok &= (df[var].isna() & train[var].isna().any()).to_numpy() | df[var].isin(known).to_numpy()
    return df[ok].reset_index(drop=True)


def rolling_exact(t, x, window, forward):
    """Every statistic of one group from its definition, in np.longdouble: t int64 [n] ascending, x [n]; window an int (rows) or
    ('span', length in t's units).  Returns {stat: float64 [n]} (Std two-pass, ddof 1)."""
    n = len(t)
    out = {st: np.full(n, np.nan) for st in STATS}
    for i in range(n):
        if isinstance(window, tuple):             # backward (t - span, t], forward [t, t + span)
            lo = i if forward else int(np.searchsorted(t, t[i] - window[1], side='right'))
            hi = int(np.searchsorted(t, t[i] + window[1], side='left')) - 1 if forward else i
        else:
            lo, hi = (i, min(n - 1, i + window - 1)) if forward else (max(0, i - window + 1), i)
        v = x[lo:hi + 1]
        v = v[~np.isnan(v)].astype(np.longdouble)
        out['Count'][i] = len(v)
        if len(v) >= 1:
            s = v.sum(dtype=np.longdouble)
            out['Sum'][i], out['Min'][i], out['Max'][i], out['Mean'][i] = float(s), float(v.min()), float(v.max()), float(s / len(v))
        if len(v) >= 2:
            m = s / len(v)
            out['Std'][i] = float(np.sqrt(((v - m) ** 2).sum(dtype=np.longdouble) / (len(v) - 1)))
    return out


def exact_like(ref, t_of_row, group_of_row, values, window):
    "`rolling_exact` laid out as the reference's frame `ref` (one row per (group, time)): {column name: float64 [rows]}"
    out = {c: np.full(len(ref), np.nan) for c in ref.columns if 'Roll' in c}
    for g in pd.unique(group_of_row):
        rows = np.where(group_of_row == g)[0]
        assert (np.diff(t_of_row[rows]) > 0).all()
        for col in ROLL_COLS:
            for fwd, tag in ((False, 'RollBwd'), (True, 'RollFwd')):
                ex = rolling_exact(t_of_row[rows], values[col][rows], window, fwd)
                for st in STATS:
                    out[col + tag + st][rows] = ex[st]
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype='float64').view('int64'), np.asarray(b, dtype='float64').view('int64')) or \
        bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def check_rolling(tag, ref, exact, values, longest, out):
    "values: {column: the input values}; the bound on the reference's Sum / Mean is per column: longest 2^-52 max|x|"
    d = {'Sum': 0.0, 'Mean': 0.0, 'Std': 0.0}
    for name, ex in exact.items():
        r = ref[name].to_numpy(dtype='float64')
        st = [s for s in STATS if name.endswith(s)][0]
        col = [c for c in ROLL_COLS if name.startswith(c + 'Roll')][0]
        assert np.array_equal(np.isnan(r), np.isnan(ex)), (tag, name, 'NaN positions')
        if st in ('Min', 'Max', 'Count') or (st == 'Sum' and col == 'k'):
            assert same_bits(r, ex), (tag, name, 'not bit-equal to the definition')
        if st in d:
            dist = float(np.nanmax(np.abs(r - ex)))
            d[st] = max(d[st], dist)
            if st != 'Std':
                bound = longest * 2.0 ** -52 * float(np.nanmax(np.abs(values[col])))
                assert dist <= bound, (tag, name, dist, bound)
        out['%s.roll.%s' % (tag, name)] = r
        out['%s.roll.%s_exact' % (tag, name)] = ex
    print('%s: d_Sum %.3e d_Mean %.3e d_Std %.3e' % (tag, d['Sum'], d['Mean'], d['Std']), flush=True)
    for st, v in d.items():
        out['%s.roll.d_%s' % (tag, st)] = np.float64(v)
    out['%s.roll.columns' % tag] = np.array(list(ref.columns))


def frame_arrays(prefix, df, out, skip=()):
    "a frame as arrays: datetimes as int64 nanoseconds, strings as unicode ('nan' for missing)"
    out[prefix + '.index'] = np.asarray(df.index.view('int64') if isinstance(df.index, pd.DatetimeIndex) else df.index)
    out[prefix + '.columns'] = np.array(list(df.columns))
    for c in df.columns:
        if c in skip:
            continue
        v = df[c]
        if pd.api.types.is_datetime64_any_dtype(v):
            out['%s.col.%s' % (prefix, c)] = v.to_numpy().astype('datetime64[ns]').view('int64')
        elif v.dtype == object:
            out['%s.col.%s' % (prefix, c)] = v.astype(str).to_numpy(dtype='U')
        else:
            out['%s.col.%s' % (prefix, c)] = v.to_numpy()


def part_ab(out, SD):
    A = frame_a()
    frame_arrays('a.in', A, out)
    before = A.copy()
    for ev in ('Promo', 'Holiday'):
        tba = SD.get_TimeBeforeAfter(A.copy(), ev, index_col='Date', groupby_col='Store', timescale=DAY)
        frame_arrays('a.tba.' + ev, tba, out)
        assert tba[ev + 'Before'].notna().any() and tba[ev + 'After'].notna().any()
    roll = SD.get_RollingStats(A.copy(), ROLL_COLS, '8D', STATS, index_col='Date', groupby_col='Store')
    assert A.equals(before)
    t = roll.index.view('int64')
    S = A.set_index(['Store', 'Date'])
    values = {c: S.loc[list(zip(roll['Store'], roll.index)), c].to_numpy() for c in ROLL_COLS}
    exact = exact_like(roll, t, roll['Store'].to_numpy(), values, ('span', 8 * 86400 * 10 ** 9))
    out['a.roll.index'] = t
    out['a.roll.Store'] = roll['Store'].to_numpy()
    out['a.roll.index_col'] = roll['index'].to_numpy().astype('datetime64[ns]').view('int64')
    check_rolling('a', roll, exact, values, max(A_SIZES), out)
    alone = roll[roll['Store'] == 11]
    assert len(alone) == 1 and np.isnan(alone['xRollBwdSum'].iloc[0]) and alone['xRollFwdCount'].iloc[0] == 0

    B = frame_b()
    frame_arrays('b.in', B, out)
    tba = SD.get_TimeBeforeAfter(B.copy(), 'E', timescale=1)
    frame_arrays('b.tba.E', tba, out)
    roll = SD.get_RollingStats(B.copy(), ROLL_COLS, 3, STATS)
    t = np.asarray(roll.index, dtype='int64')
    values = {c: B.loc[roll.index, c].to_numpy() for c in ROLL_COLS}
    exact = exact_like(roll, t, np.zeros(len(t), dtype='int64'), values, 3)
    out['b.roll.index'] = t
    check_rolling('b', roll, exact, values, len(B), out)


def labels_arrays(prefix, category_labels, out):
    out[prefix + '.n'] = np.int64(len(category_labels))
    for j, d in enumerate(category_labels):
        out['%s.%d.keys' % (prefix, j)] = np.array([str(k) for k in d.keys()])
        out['%s.%d.values' % (prefix, j)] = np.array(list(d.values()), dtype='int64')


def processed_arrays(prefix, res, out):
    xcat, xcont, y, scaling, labels = res
    out[prefix + '.xcat'] = xcat.to_numpy().astype('int64')
    out[prefix + '.xcont'] = xcont.to_numpy().astype('float32')
    assert xcont.to_numpy().dtype == np.float32
    if y is not None:
        out[prefix + '.y'] = np.asarray(y)
    out[prefix + '.index'] = np.asarray(xcat.index)
    return scaling, labels


def part_c(out, SD):
    train, val, test = process_frames()
    for tag, cat_vars, cont_vars, target, unknown, frames in (
            ('c', CAT_VARS, CONT_VARS, 'target', True, (train, val, test)),
            ('c2', CAT_VARS2, CONT_VARS2, 'label', False, (train, seen_rows(val, train), seen_rows(test, train)))):
        tr, va, te = frames
        assert len(va) >= 5 and len(te) >= 4, (tag, len(va), len(te))
        res = SD.ProcessDataFrame(tr.copy(), cat_vars, cont_vars, target, 'by_df', 'median', None, unknown)
        scaling, labels = processed_arrays(tag + '.train', res, out)
        labels_arrays(tag + '.labels', labels, out)
        out[tag + '.scaling.vars'] = np.array(list(scaling.keys()))
        out[tag + '.scaling'] = np.array([[float(m), float(s)] for m, s in scaling.values()], dtype='float64')
        res = SD.ProcessDataFrame(va.copy(), cat_vars, cont_vars, target, scaling, 'median', labels, unknown)
        processed_arrays(tag + '.val', res, out)
        xcat_vars, xcont_vars = [v for v in cat_vars if v != target], [v for v in cont_vars if v != target]
        res = SD.ProcessDataFrame(te.copy(), xcat_vars, xcont_vars, None, scaling, 'median', labels, unknown)
        processed_arrays(tag + '.test', res, out)
        out[tag + '.rows'] = np.array([len(tr), len(va), len(te)])
        print(tag, 'labels', labels, flush=True)
    if (out['c.val.xcat'] == 0).sum() < 3:
        raise AssertionError('(c): val holds too few missing / unseen categorical values')


def part_d(out):
    A = frame_a()
    d = pd.to_datetime(A['Date']).dt
    exp = {'week': d.isocalendar().week, 'month': d.month, 'year': d.year, 'dayofweek': d.dayofweek, 'dayofmonth': d.day,
           'dayofyear': d.dayofyear, 'is_month_end': d.is_month_end, 'is_month_start': d.is_month_start, 'is_quarter_end': d.is_quarter_end,
           'is_quarter_start': d.is_quarter_start, 'is_year_end': d.is_year_end, 'is_year_start': d.is_year_start}
    for name in DATEPART[:-1]:
        out['d.' + name] = exp[name].to_numpy().astype('int64')
    out['d.days_elapsed'] = ((A['Date'] - A['Date'].min()) / DAY).to_numpy().astype('float64')
    out['d.days_elapsed_from_2014'] = ((A['Date'] - pd.Timestamp('2014-12-25')) / DAY).to_numpy().astype('float64')


def main():
    from oracle import _ref_import
    SD = _ref_import.load()['Applications.StructuredData']
    SD.PBar = lambda it, *a, **k: it
    out = {}
    part_ab(out, SD)
    part_c(out, SD)
    part_d(out)
    np.savez_compressed(OUT, **out)
    with np.load(OUT, allow_pickle=False) as z:
        assert len(z.files) == len(out)
    print('wrote', OUT, '%.1f KB' % (os.path.getsize(OUT) / 1024), len(out), 'arrays')


if __name__ == '__main__':
    main()
