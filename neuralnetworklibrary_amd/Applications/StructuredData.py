"""Structured (tabular) data application of the drop-in API: Applications/StructuredData.py §1.3 (feature engineering: add_datepart
:432, get_TimeBeforeAfter :460, get_RollingStats :530) and §2 (ProcessDataFrame :614, StructuredDataset :803, StructuredDataCollater
:849, StructuredDataObj :871 with from_dataframes :913, embedding_dim :970, StructuredDataNet :979-1096, StructuredDataEnsembleNet :1098).

HIP-backed hot paths.  Model: the categorical front end (per-column max_norm renorm + gather + per-sample dropout + both torch.cat
calls) is ONE fused gather kernel (ops.tab_embed_concat, K3) and one scatter-add kernel in backward; the FC head runs on the fp32-MFMA
GEMM (ops.linear) and the fused BatchNorm kernels (ops.bn_act).  Data: the two slow cells of the Rossmann notebook, the per-row Python
loop of get_TimeBeforeAfter and the per-group pandas rolling of get_RollingStats, are scans over rows sorted by (group, time) on the
device (ops.seg_event_gaps, ops.seg_rolling, K12); like every op they need a GPU and have no CPU fallback.  add_datepart and
ProcessDataFrame are host pandas: calendar fields pandas already has, and string work that runs once, offline.  EDA (§1.2, :235-428):
missing_value_counts, the entropy / correlation-ratio / correlation helpers, get_association, associations_dependent and
associations_pairs compute all pairs of a call on the device (ops.assoc_*, K13: contingency counts and fp64 moments).
Still out of scope: the EDA plots (plot_distributions, plot_dependence, plot_pairs) and CSV reading.
"""
import numpy as np
import pandas as pd
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.data import Dataset, DataLoader

from ..General.Core import *          # noqa: F401,F403
from ..General.Layers import *        # noqa: F401,F403
from ..General.Learner import *       # noqa: F401,F403
from ..General.LossesMetrics import * # noqa: F401,F403
from ..General.Optimizer import *     # noqa: F401,F403
from ..General.Core import TEN, separate_bn_layers
from ..General.Layers import EmbeddingDrop, Flatten1d, FullyConnectedNet
from .. import ops
from ..dist import keyed_mask


# ---- §1.2 EDA: numerical measures of association (StructuredData.py:235-428) --------------------------------------------------
# One call = one upload of the distinct columns the requested pairs use (categorical columns factorised to int32 codes, -1 for
# missing; continuous ones as float64 with NaN for missing and one shift, the column's nanmean), the K13 kernels over all pairs
# (ops.assoc_*), and one small copy back of a few numbers per pair.  Contingency tables and per-category moments stay on the device.
#
# Deliberate differences from the reference: the six direct helpers raise ValueError on a missing value, naming the column (the
# reference "assumes" there is none, and its entropy then divides by the wrong length); +-inf in a continuous column raises
# ValueError before anything is uploaded; in abs_max_correlation |X - mean(X)| counts as constant, and its correlations are skipped
# as pandas' NaN ones are, when its centred sum of squares is at most n (2^-26 mean|X - mean(X)|)^2 (our pair mean is not bit-equal to
# pandas', so a column such as balanced +-1, exactly constant there, would otherwise yield a correlation of rounding noise; 2^-26
# is the geometric middle between rounding noise, 2^-52, and a data-sized spread); an unknown Type raises ValueError; no frame is
# modified; nothing is printed; plot=True is written fresh (a pandas bar plot, a seaborn heatmap with the diagonal zeroed).
# correlation_ratio and max_correlation_ratio sum per category with fp64 atomics: their last bits may differ between calls; the
# entropy- and correlation-based measures are bit-equal from call to call.

ASSOCIATION_TYPES = {'abs_correlation': 'cont', 'abs_max_correlation': 'cont', 'correlation_ratio': 'cat_cont',
                     'max_correlation_ratio': 'cat_cont', 'mutual_info_asymmetric': 'cat', 'mutual_info_symmetric': 'cat'}
_ASSOC_CHUNK_CELLS = 2 ** 25             # contingency cells per ops call: bounds the table workspace at 128 MiB
_ONE = object()                          # a stand-in column with one category: H_X alone is the table stats of (X, _ONE)


def missing_value_counts(df):
    "Counts of missing values in the columns of df that have any (StructuredData.py:235-238).  Host pandas."
    counts = df.isnull().astype(int).sum()
    return counts[counts > 0]


def _assoc_device():
    from .._lib import NnlError
    if not torch.cuda.is_available():
        raise NnlError('the association measures run on the GPU (ops.assoc_*): there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _assoc_upload(df, cat_cols, cont_cols, strict):
    """The host half: factorise / convert the distinct columns and upload them in ONE buffer.
    -> (codes int32 [Vc, n] or None, card, vals float64 [Vy, n] or None, shift float64 [Vy] or None)"""
    n = len(df)
    if n < 1:
        raise ValueError('the frame has no rows')
    codes, card, vals = [], [], []
    for col in cat_cols:
        if col is _ONE:
            codes.append(np.zeros(n, dtype=np.int32)), card.append(1)
            continue
        c, uniques = pd.factorize(df[col])
        if strict and (c < 0).any():
            raise ValueError('column %r holds missing values' % (col,))
        codes.append(c.astype(np.int32)), card.append(max(len(uniques), 1))
    for col in cont_cols:
        v = df[col].to_numpy(dtype='float64', na_value=np.nan)
        if np.isinf(v).any():
            raise ValueError('column %r holds an infinite value' % (col,))
        if strict and np.isnan(v).any():
            raise ValueError('column %r holds missing values' % (col,))
        vals.append(v)
    shifts = [float(np.nanmean(v)) if not np.isnan(v).all() else 0.0 for v in vals]
    dev = _assoc_device()
    Vc, Vy = len(codes), len(vals)
    buf = np.empty(8 * Vy * (n + 1) + 4 * Vc * n, dtype=np.uint8)
    if Vy:
        buf[:8 * Vy * n].view(np.float64).reshape(Vy, n)[:] = np.stack(vals)
        buf[8 * Vy * n:8 * Vy * (n + 1)].view(np.float64)[:] = shifts
    if Vc:
        buf[8 * Vy * (n + 1):].view(np.int32).reshape(Vc, n)[:] = np.stack(codes)
    d = torch.from_numpy(buf).to(dev)
    d_vals = d[:8 * Vy * n].view(torch.float64).view(Vy, n) if Vy else None
    d_shift = d[8 * Vy * n:8 * Vy * (n + 1)].view(torch.float64) if Vy else None
    d_codes = d[8 * Vy * (n + 1):].view(torch.int32).view(Vc, n) if Vc else None
    return d_codes, np.asarray(card, dtype=np.int64), d_vals, d_shift


def _distinct(items):
    seen = {}
    for it in items:
        seen.setdefault(it, len(seen))
    return list(seen), seen


def _assoc_prepare(df, pairs, family, strict=False):
    "host half of one call: the distinct columns of `pairs` on the device and the pairs as column indices"
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    if family == 'cat_cont':
        ccols, cwhere = _distinct(xs)
        ycols, ywhere = _distinct(ys)
        codes, card, vals, shift = _assoc_upload(df, ccols, ycols, strict)
        return codes, card, vals, shift, np.array([cwhere[x] for x in xs]), np.array([ywhere[y] for y in ys])
    cols, where = _distinct(xs + ys)
    codes, card, vals, shift = _assoc_upload(df, cols if family == 'cat' else [], cols if family == 'cont' else [], strict)
    px, py = np.array([where[x] for x in xs]), np.array([where[y] for y in ys])
    if family == 'cat':
        cells = card[px] * card[py]
        if cells.max() > ops.ASSOC_MAX_TABLE_CELLS:
            k = int(cells.argmax())
            raise ValueError('the contingency table of %r x %r has %d cells, above the limit of %d'
                             % (xs[k], ys[k], cells[k], ops.ASSOC_MAX_TABLE_CELLS))
    return codes, card, vals, shift, px, py


def _assoc_run(prepared, family, with_abs=True):
    "device half: the K13 kernels over all pairs -> float64 [P, K] on the device"
    codes, card, vals, shift, px, py = prepared
    if family == 'cat_cont':
        return ops.assoc_cat_cont(codes, card, vals, shift, px, py)
    if family == 'cont':
        return ops.assoc_cont_cont(vals, shift, px, py, with_abs=with_abs)
    cells = card[px] * card[py]
    out, lo = [], 0
    while lo < len(px):                         # chunks of the pair list: the table workspace stays bounded
        hi = lo + 1
        while hi < len(px) and cells[lo:hi + 1].sum() <= _ASSOC_CHUNK_CELLS:
            hi += 1
        tables, offsets = ops.assoc_contingency(codes, card, px[lo:hi], py[lo:hi])
        out.append(ops.assoc_table_stats(tables, card, px[lo:hi], py[lo:hi], offsets))
        lo = hi
    return torch.cat(out)


def _assoc_stats(df, pairs, family, with_abs=True, strict=False):
    """Per-pair statistics of one family as a float64 numpy array [P, K] (see ops.assoc_table_stats, ops.assoc_cat_cont,
    ops.assoc_cont_cont): one upload, the kernels, one copy back."""
    return _assoc_run(_assoc_prepare(df, pairs, family, strict), family, with_abs).cpu().numpy()


def _association_values(df, pairs, Type):
    "get_association for every (X, Y) of `pairs`, as a list of floats: the reference's short-circuits, one device call for the rest"
    if Type not in ASSOCIATION_TYPES:
        raise ValueError('Type must be one of %s (got %r)' % (sorted(ASSOCIATION_TYPES), Type))
    family = ASSOCIATION_TYPES[Type]
    values = [1.0 if x == y else None for x, y in pairs]
    todo = [k for k, v in enumerate(values) if v is None]
    if not todo:
        return values
    if len(df) == 0:
        return [0.0 if v is None else v for v in values]
    st = _assoc_stats(df, [pairs[k] for k in todo], family, with_abs=(Type == 'abs_max_correlation'))
    for k, s in zip(todo, st):
        if family == 'cat':
            n, rows, cols, hx, hy, hxy = s
            if n == 0 or rows == 1 or cols == 1:
                values[k] = 0.0
            else:
                i_xy = hx + hy - hxy
                values[k] = float(i_xy / hy if Type == 'mutual_info_asymmetric' else 0.5 * (i_xy / hx + i_xy / hy))
        elif family == 'cat_cont':
            n, cats, ratio, max_ratio, ymin, ymax = s
            if n == 0 or cats == 1 or ymin == ymax:
                values[k] = 0.0
            else:
                values[k] = float(ratio if Type == 'correlation_ratio' else min(max_ratio / 3, 1.0))
        else:
            n, degenerate, c1, cmax = s
            values[k] = 0.0 if degenerate else float(c1 if Type == 'abs_correlation' else cmax)
    return values


def _divide(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.float64(a) / np.float64(b))


def entropy(df, X):
    """Entropy (natural log) of the categorical column X of df (StructuredData.py:240-244).  Raises ValueError if X holds a missing
    value (the reference assumes there is none and would divide by the wrong length)."""
    return float(_assoc_stats(df, [(X, _ONE)], 'cat', strict=True)[0, 3])


def joint_entropy(df, X, Y):
    """Joint entropy of the categorical columns X, Y (:246-252), with the reference's clamp: every empty cell of the observed
    categories' table adds -1e-20 log(1e-20).  Raises ValueError on a missing value."""
    return float(_assoc_stats(df, [(X, Y)], 'cat', strict=True)[0, 5])


def normed_mutual_info(df, X, Y, symmetric):
    """I(X;Y)/H(Y), or symmetric: 0.5 (I(X;Y)/H(X) + I(X;Y)/H(Y)) (:254-262).  Raises ValueError on a missing value."""
    _, _, _, hx, hy, hxy = _assoc_stats(df, [(X, Y)], 'cat', strict=True)[0]
    i_xy = hx + hy - hxy
    return 0.5 * (_divide(i_xy, hx) + _divide(i_xy, hy)) if symmetric else _divide(i_xy, hy)


def correlation_ratio(df, X, Y):
    """Correlation ratio of categorical X and numeric Y (:264-271): the between-category sum of squares is divided by n, the variance
    of Y is the ddof=1 one.  Raises ValueError on a missing or infinite value.  Last bits may differ between calls (fp64 atomics)."""
    return float(_assoc_stats(df, [(X, Y)], 'cat_cont', strict=True)[0, 2])


def max_correlation_ratio(df, X, Y):
    """max_i |mean(Y | X = x_i) - mean(Y)| / std(Y) (:273-287), raw: in [0, inf).  Raises ValueError on a missing or infinite value.
    Last bits may differ between calls (fp64 atomics)."""
    return float(_assoc_stats(df, [(X, Y)], 'cat_cont', strict=True)[0, 3])


def abs_max_correlation(df, X, Y):
    """max(|c1|, |c2|, |c3|, |c4|) with c1 = corr(X, Y), c2 = corr(X, Y2), c3 = corr(X2, Y), c4 = corr(X2, Y2), X2 = |X - mean(X)|,
    Y2 = |Y - mean(Y)| (:289-309).  A correlation with a constant X2 or Y2 (NaN in pandas) is skipped; X2 counts as constant when its
    centred sum of squares is at most n (2^-26 mean(X2))^2.  Raises ValueError on a missing or infinite value; NaN if X or Y is constant."""
    return float(_assoc_stats(df, [(X, Y)], 'cont', strict=True)[0, 3])


def get_association(df, X, Y, Type):
    """Unsigned association strength of X and Y in [0, 1] (:311-338).  Type: 'abs_correlation' / 'abs_max_correlation' (both numeric),
    'correlation_ratio' / 'max_correlation_ratio' (X categorical, Y numeric; the latter as min(ratio / 3, 1)),
    'mutual_info_symmetric' / 'mutual_info_asymmetric' (both categorical).  X == Y gives 1.0; the rows are those where both are
    present; no such row, or a single distinct value in either column on those rows, gives 0.0."""
    return _association_values(df, [(X, Y)], Type)[0]


def _need(module, what):
    import importlib
    try:
        return importlib.import_module(module)
    except ImportError as e:
        raise ImportError('plot=True needs %s for %s, which is not installed (pass plot=False)' % (module.split('.')[0], what)) from e


def associations_dependent(df, Type, variables, depend_var, reverse=False, plot=True):
    """Association of each of `variables` with depend_var (reverse: of depend_var with each) as a pd.Series indexed by `variables`,
    optionally as a bar plot (:340-359).  One device call for all variables."""
    variables = list(variables)
    pairs = [(depend_var, v) if reverse else (v, depend_var) for v in variables]
    associations = pd.Series(_association_values(df, pairs, Type), index=variables, dtype='float64')
    if plot:
        _need('matplotlib.pyplot', 'the bar plot')
        figsize = (len(associations) / 2, max(len(associations) / 4, 4))
        associations.plot.bar(title='Associations with ' + str(depend_var), figsize=figsize)
    return associations


def associations_pairs(df, Type, cat_vars=None, cont_vars=None, plot=True):
    """Associations between pairs of variables as a pd.DataFrame, optionally as a heatmap (:361-428).  cat_vars and cont_vars: rows
    cat_vars, columns cont_vars; cat_vars alone or cont_vars alone: all ordered pairs of that list.  One device call for all pairs."""
    if cat_vars and cont_vars:
        rows, cols = list(cat_vars), list(cont_vars)
    elif cont_vars is None:
        rows = cols = list(cat_vars)
    elif cat_vars is None:
        rows = cols = list(cont_vars)
    else:
        raise ValueError('give cat_vars, cont_vars or both')
    values = _association_values(df, [(x, y) for x in rows for y in cols], Type)
    Assoc = pd.DataFrame(np.asarray(values, dtype='float64').reshape(len(rows), len(cols)), index=rows, columns=cols)
    if plot:
        _need('matplotlib.pyplot', 'the heatmap')
        sns = _need('seaborn', 'the heatmap')
        shown = Assoc if rows is not cols else Assoc - pd.DataFrame(np.identity(len(rows)), index=rows, columns=cols)
        heatmap = sns.heatmap(shown, cbar_kws={'shrink': .5}, cmap='Reds', fmt='.2f', square=True, linewidths=.5, annot=True,
                              xticklabels=cols, yticklabels=rows)
        heatmap.figure.set_size_inches(len(rows), 1.5 * len(cols))
        sns.despine()
    return Assoc


# ---- §1.3 feature engineering ------------------------------------------------------------------------------------------

def add_datepart(df, date_column='Date', start=None):
    """Adds 'week', 'month', 'year', 'dayofweek', 'dayofmonth', 'dayofyear', 'is_month_end/start', 'is_quarter_end/start',
    'is_year_end/start' (integer columns) and 'days_elapsed' (days since `start`, default the earliest date) to df, in place
    (StructuredData.py:432-458).  Host pandas: one pass over calendar fields pandas already has.  'week' is the ISO week
    (.dt.isocalendar().week: the reference's .dt.week, which current pandas no longer has)."""
    df[date_column] = pd.to_datetime(df[date_column])
    d = df[date_column].dt
    df['week'] = d.isocalendar().week.astype('int64')
    df['month'], df['year'] = d.month, d.year
    df['dayofweek'], df['dayofmonth'], df['dayofyear'] = d.dayofweek, d.day, d.dayofyear
    for name in ('is_month_end', 'is_month_start', 'is_quarter_end', 'is_quarter_start', 'is_year_end', 'is_year_start'):
        df[name] = getattr(d, name).astype(int)
    if start is None:
        start = df[date_column].min()
    df['days_elapsed'] = (df[date_column] - pd.to_datetime(start)) / np.timedelta64(1, 'D')


def _time_values(values, what):
    "times as int64: nanoseconds of a datetime column / index, or the integer index itself -> (t [n], is_datetime)"
    values = pd.Series(np.asarray(values) if not isinstance(values, (pd.Series, pd.Index)) else values).reset_index(drop=True)
    if values.isna().any():
        raise ValueError('%s holds NaT / NaN: every row needs a time' % what)
    if pd.api.types.is_datetime64_any_dtype(values):
        if getattr(values.dt, 'tz', None) is not None:
            values = values.dt.tz_convert('UTC').dt.tz_localize(None)
        return values.to_numpy().astype('datetime64[ns]').view('int64'), True
    if pd.api.types.is_integer_dtype(values):
        return values.to_numpy().astype('int64'), False
    if pd.api.types.is_float_dtype(values) and (values == np.floor(values)).all():
        return values.to_numpy().astype('int64'), False
    raise ValueError('%s must hold timestamps or integers (got dtype %s)' % (what, values.dtype))


def _sorted_rows(df, index_col, groupby_col):
    """The host half of the scans: `order` = positions of df's rows sorted by (group label, time) — groups in sorted label order, rows
    of a missing label dropped, as groupby does —, t int64 and head uint8 in that order.  Duplicate times inside a group raise."""
    what = repr(index_col) if index_col is not None else 'the index'
    t, is_dt = _time_values(df[index_col] if index_col is not None else df.index, what)
    if len(t) == 0:
        raise ValueError('the frame has no rows')
    if groupby_col is None:
        codes, order = np.zeros(len(t), dtype='int64'), np.argsort(t, kind='stable')
    else:
        # the order of np.lexsort((t, codes)), by ONE integer key where it fits: group code x number of distinct times + rank of the time
        # (two hash factorisations and one sort of int64 keys: a third of the lexsort's time at a million rows)
        codes = pd.factorize(df[groupby_col], sort=True)[0].astype('int64')
        ranks, distinct = pd.factorize(t, sort=True)
        if (int(codes.max()) + 1) * len(distinct) < 2 ** 62:
            order = np.argsort(codes * len(distinct) + ranks)       # equal keys are duplicate times: they raise below
        else:
            order = np.lexsort((t, codes))
    codes = codes[order]
    if codes[0] < 0:                                                # rows without a group label sort first: dropped
        order, codes = order[codes >= 0], codes[codes >= 0]
        if len(order) == 0:
            raise ValueError('no row of the frame has a group label')
    t = t[order]
    head = np.ones(len(t), dtype='uint8')
    head[1:] = codes[1:] != codes[:-1]
    if ((t[1:] == t[:-1]) & (head[1:] == 0)).any():
        raise ValueError('duplicate times in %s inside a group: the rows of a group need distinct times' % what)
    return order, np.ascontiguousarray(t), head, is_dt


def _to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(default_device())


def get_TimeBeforeAfter(df, event_col, index_col=None, groupby_col=None, keep_cols=[], timescale=1):
    """Time since the last and until the next event (event_col == 1) for every row, per label of groupby_col if given, in units of
    `timescale` (a number, or an np.timedelta64 / pd.Timedelta for timestamps); NaN where there is no such event; a row's own event does
    not count (StructuredData.py:460-519).  Returns the reference's frame: columns [index_col or 'index', *keep_cols, (groupby_col),
    event_col + 'Before', event_col + 'After'], groups in sorted label order, time ascending inside a group, df's index kept.
    The host factorises and sorts by (group, time), the order of np.lexsort; the two scans are one ops.seg_event_gaps call on the device.
    The times of a group must be distinct and none may be missing (ValueError; the reference's NOTE 2).  Unlike the reference, which
    adds and drops an 'index' column on it, df is not modified."""
    order, t, head, is_dt = _sorted_rows(df, index_col, groupby_col)
    if isinstance(timescale, (np.timedelta64, pd.Timedelta)):
        timescale = pd.Timedelta(timescale).value
    event = (df[event_col].to_numpy()[order] == 1).astype('uint8')
    before, after, _, _ = ops.seg_event_gaps(_to_device(t), _to_device(head), _to_device(event), float(timescale))
    gaps = torch.stack([before, after]).cpu().numpy()
    keep = list(keep_cols) + ([groupby_col] if groupby_col is not None else [])
    if index_col is None:
        out = pd.DataFrame({'index': df.index[order]}, index=df.index[order])
        for c in keep:
            out[c] = df[c].to_numpy()[order]
    else:
        out = df[[index_col] + keep].iloc[order].copy()
    out[event_col + 'Before'], out[event_col + 'After'] = gaps[0], gaps[1]
    return out


def get_RollingStats(df, columns, window_size, stat_types, index_col=None, groupby_col=None, keep_cols=[]):
    """Backward and forward rolling statistics ('Sum', 'Min', 'Max', 'Mean', 'Std', 'Count') of the numeric `columns`, per label of
    groupby_col if given (StructuredData.py:530-607).  window_size: an int (rows), or anything pd.Timedelta parses ('8D': needs a
    datetime index / index_col): backward the rows in (t - window, t], forward those in [t, t + window).  Returns the reference's
    frame: indexed by time, for each statistic all c + 'RollBwd' + st columns, then all c + 'RollFwd' + st; when grouped, groupby_col
    and 'index' are appended and the groups follow each other in sorted label order.  keep_cols is ignored (the reference uses it
    only when it calls itself).  One upload, one ops.seg_event_gaps call for the group bounds, two ops.seg_rolling calls and one copy
    back: each output costs O(window) on the device.  Restriction: the times of a group must be distinct and none may be missing
    (ValueError).  df is not modified."""
    order, t, head, is_dt = _sorted_rows(df, index_col, groupby_col)
    stats = list(stat_types)
    if isinstance(window_size, (int, np.integer)) and not isinstance(window_size, bool):
        window = dict(count_window=int(window_size))
    else:
        if not is_dt:
            raise ValueError('a time window (%r) needs a datetime index' % (window_size,))
        window = dict(span=pd.Timedelta(window_size).value)
    if min(window.values()) < 1:
        raise ValueError('window_size must be positive (got %r)' % (window_size,))
    x = np.stack([df[c].to_numpy(dtype='float64')[order] for c in columns])
    td = _to_device(t)
    _, _, seg_start, seg_end = ops.seg_event_gaps(td, _to_device(head), torch.zeros(len(t), dtype=torch.uint8, device=td.device))
    xd = _to_device(x)
    both = torch.stack([ops.seg_rolling(td, seg_start, seg_end, xd, stats, forward=fwd, **window) for fwd in (False, True)])
    both = both.cpu().numpy()                                           # [direction, statistic, column, row]
    times = (df[index_col] if index_col is not None else df.index).to_numpy()[order]
    index = pd.Index(times, name=index_col if index_col is not None else df.index.name)
    data = {}
    for s, st in enumerate(stats):
        for d, tag in enumerate(('RollBwd', 'RollFwd')):
            for c, col in enumerate(columns):
                data[col + tag + st] = both[d, s, c]
    out = pd.DataFrame(data, index=index)
    if groupby_col is not None:
        out[groupby_col] = df[groupby_col].to_numpy()[order]
        out['index'] = out.index
    return out


# ---- §2.1 data object construction ---------------------------------------------------------------------------------------

_MISSING = 'nan'          # how the reference spells a missing categorical value (astype(str) of np.nan)


def _category_strings(col):
    "a categorical column as strings: float-coded integers through int (7.0 -> '7'), missing values (None, NaN) -> 'nan'"
    missing = col.isna().to_numpy()
    if pd.api.types.is_float_dtype(col):
        s = col.fillna(0).astype('int64').astype(str).to_numpy(dtype=object)
    else:
        s = col.astype(str).to_numpy(dtype=object)
    s[missing] = _MISSING
    return s


def ProcessDataFrame(df, cat_vars, cont_vars, output_var, scale_cont, fill_missing='median', category_labels=None, unknown_category=True):
    """DataFrame -> (xcat_df, xcont_df, y, scaling_values, category_labels) with the reference's semantics (StructuredData.py:614-801).

    cat_vars hold strings or (possibly float-coded) integers; the categories of a variable are the lexicographically sorted string
    forms of its values.  unknown_category=True: missing values become 0 ('unknown') and the known categories 1, 2, ...; values not
    in `category_labels` (unseen validation / test values) become 0 as well.  unknown_category=False: the categories become 0, 1, ...
    (a missing value is then a category of its own, 'nan'; a value without a label raises).  A categorical output is numbered in
    order of first appearance.  cont_vars are cast to float32, filled (fill_missing = 'median', 'mean' or a constant), then scaled:
    scale_cont = 'No', 'by_df' (this frame's mean and std, returned as scaling_values[var] = [mean, std]) or such a dictionary.
    category_labels: None for the training frame, otherwise what the call on the training frame returned.
    Host code: this is string work and runs once, offline.  None and NaN both count as missing.  df is not modified (the reference
    converts its columns in place)."""
    xcat_vars = [v for v in cat_vars if v != output_var]
    xcont_vars = [v for v in cont_vars if v != output_var]
    need_labels = category_labels is None
    category_labels = [] if need_labels else category_labels

    def codes_of(strings, labels, var):
        codes = pd.Series(strings).map(labels)
        if unknown_category and 'unknown' in labels:
            codes = codes.fillna(labels['unknown'])
        if codes.isna().any():
            raise ValueError('%r holds values without a category label: %s' % (var, sorted(set(strings[codes.isna().to_numpy()]))[:5]))
        return codes.to_numpy().astype('int64')

    y = None
    y_labels = None
    if output_var is not None and output_var in cont_vars:
        y = df[output_var].to_numpy(dtype='float32')
    elif output_var is not None and output_var in cat_vars:
        s = _category_strings(df[output_var])
        if need_labels:
            y_labels = {c: i for i, c in enumerate(pd.unique(s))}
        labels = y_labels if need_labels else category_labels[-1]
        if not all(c in labels for c in pd.unique(s)):
            raise ValueError('%r holds values without a category label' % output_var)
        y = pd.Series(s).map(labels).to_numpy().astype('int64')

    xcat_df = None
    if xcat_vars:
        cols = {}
        for j, var in enumerate(xcat_vars):
            s = _category_strings(df[var])
            if need_labels:
                cats = sorted(set(s) - {_MISSING}) if unknown_category else sorted(set(s))
                labels = {c: i + 1 for i, c in enumerate(cats)} if unknown_category else {c: i for i, c in enumerate(cats)}
                if unknown_category:
                    labels['unknown'] = 0
                category_labels.append(labels)
            labels = category_labels[j]
            cols[var] = codes_of(s, labels, var)
        xcat_df = pd.DataFrame(cols, index=df.index, columns=xcat_vars)
    if need_labels and y_labels is not None:
        category_labels.append(y_labels)

    scaling_values = None
    if xcont_vars and isinstance(scale_cont, str) and scale_cont == 'by_df':
        scaling_values = {}
    elif xcont_vars and isinstance(scale_cont, dict):
        scaling_values = scale_cont
    xcont_df = None
    if xcont_vars:
        xcont_df = df[xcont_vars].astype('float32')
        if isinstance(fill_missing, str) and fill_missing == 'median':
            xcont_df = xcont_df.fillna(xcont_df.median())
        elif isinstance(fill_missing, str) and fill_missing == 'mean':
            xcont_df = xcont_df.fillna(xcont_df.mean())
        else:
            xcont_df = xcont_df.fillna(pd.Series(fill_missing, index=xcont_vars))
        if scaling_values is not None:
            for var in xcont_vars:
                if not isinstance(scale_cont, dict):
                    scaling_values[var] = [xcont_df[var].mean(), xcont_df[var].std()]
                mean, std = scaling_values[var]
                xcont_df[var] = (xcont_df[var] - mean) / std
        xcont_df = xcont_df.astype('float32')
    return xcat_df, xcont_df, y, scaling_values, category_labels


class StructuredDataset(Dataset):
    """x_cat int64 [N, n_cat'], x_cont float32 [N, n_cont'], y [N]; a missing block becomes a single zero column
    (Applications/StructuredData.py:803-847).  Accepts DataFrames or arrays."""

    def __init__(self, xcat_df, xcont_df, y, target_type):
        self.target_type = target_type
        L = len(xcat_df) if (xcat_df is not None) else len(xcont_df)
        self.y = y if (y is not None) else np.zeros(L).astype('float32')
        if xcat_df is not None:
            self.n_cat, self.x_cat = xcat_df.shape[1], np.array(xcat_df)
        else:
            self.n_cat, self.x_cat = 0, np.zeros((L, 1), 'int64')
        if xcont_df is not None:
            self.n_cont, self.x_cont = xcont_df.shape[1], np.array(xcont_df)
        else:
            self.n_cont, self.x_cont = 0, np.zeros((L, 1), 'float32')

    def __len__(self):
        return len(self.x_cat)

    def __getitem__(self, idx):
        return self.x_cat[idx], self.x_cont[idx], self.y[idx]

    def y_range(self):
        return [np.min(self.y), np.max(self.y)]


def StructuredDataCollater(batch):
    "list of (x_cat[i], x_cont[i], y[i]) -> [xcat, xcont], y as CPU tensors (StructuredData.py:849-869)"
    xcat = TEN(np.array([z[0] for z in batch]), GPU=False)
    xcont = TEN(np.array([z[1] for z in batch]), GPU=False)
    y = TEN(np.array([z[2] for z in batch]), GPU=False)
    return [xcat, xcont], y


class StructuredDataObj(object):
    """train / val / (test) StructuredDatasets + dataloaders (StructuredData.py:871-911).
    device_resident=True (MI355X addition): x_cat / x_cont / y live in HBM and `[xcat, xcont], y`
    minibatches are gathered on the device (device_data.DeviceBatches): no DataLoader workers, collate or per-step H2D."""

    def __init__(self, train_ds, val_ds, category_labels, scaling_values, bs, num_workers=6, test_ds=None,
                 device_resident=False, seed=0):
        self.train_ds, self.val_ds, self.test_ds = train_ds, val_ds, test_ds
        self.category_labels, self.scaling_values = category_labels, scaling_values
        self.bs, self.num_workers, self.target_type = bs, num_workers, train_ds.target_type
        if device_resident:
            from .. import dist as nnl_dist
            from ..device_data import DeviceBatches
            def mk(ds, shuffle, shard):
                y = np.asarray(ds.y)
                y = y.astype('int64') if ds.target_type == 'cat' else y.astype('float32')
                return DeviceBatches([np.asarray(ds.x_cat).astype('int64'), np.asarray(ds.x_cont).astype('float32')], y, bs,
                                     shuffle=shuffle, seed=seed, rank=nnl_dist.rank() if shard else 0,
                                     world=nnl_dist.world_size() if shard else 1)
            self.train_dl, self.val_dl = mk(train_ds, True, True), mk(val_ds, False, False)
            if self.test_ds:
                self.test_dl = mk(test_ds, False, False)
            return
        kw = dict(batch_size=bs, collate_fn=StructuredDataCollater, num_workers=num_workers, pin_memory=True)
        self.train_dl = DataLoader(train_ds, shuffle=True, **kw)
        self.val_dl = DataLoader(val_ds, shuffle=False, **kw)
        if self.test_ds:
            self.test_dl = DataLoader(test_ds, shuffle=False, **kw)

    @classmethod
    def from_dataframes(cls, train_df, val_df, cat_vars, cont_vars, output_var, bs, fill_missing='median', scale_cont=True,
                        unknown_category=True, num_workers=6, test_df=None, device_resident=False, seed=0):
        """train / val / (test) DataFrames -> data object (StructuredData.py:913-965): ProcessDataFrame on the training frame, then on
        the validation and test frames with the training frame's category labels and scaling values.  device_resident and seed go to
        the constructor.  The frames are not modified."""
        target_type = 'cat' if output_var in cat_vars else 'cont'
        xcat_vars = [v for v in cat_vars if v != output_var]
        xcont_vars = [v for v in cont_vars if v != output_var]
        xcat, xcont, y, scaling_values, category_labels = ProcessDataFrame(
            train_df, cat_vars, cont_vars, output_var, 'by_df' if scale_cont else 'No', fill_missing, None, unknown_category)
        train_ds = StructuredDataset(xcat, xcont, y, target_type)
        scale = scaling_values if scale_cont else 'No'
        xcat, xcont, y, _, _ = ProcessDataFrame(val_df, cat_vars, cont_vars, output_var, scale, fill_missing, category_labels,
                                                unknown_category)
        val_ds = StructuredDataset(xcat, xcont, y, target_type)
        test_ds = None
        if isinstance(test_df, pd.DataFrame):
            xcat, xcont, y, _, _ = ProcessDataFrame(test_df, xcat_vars, xcont_vars, None, scale, fill_missing, category_labels,
                                                    unknown_category)
            test_ds = StructuredDataset(xcat, xcont, y, target_type)
        return cls(train_ds, val_ds, category_labels, scaling_values, bs, num_workers, test_ds, device_resident=device_resident, seed=seed)


def embedding_dim(n):
    "A 'reasonable' embedding dimension for n classes (StructuredData.py:970-977)"
    if 2 <= n <= 8: return int(np.ceil(n / 2))
    if 9 <= n <= 12: return 5
    if 13 <= n <= 18: return 6
    if 19 <= n <= 27: return 7
    if 28 <= n <= 100: return int(np.ceil(n / 4))
    if n > 100: return 25


class StructuredDataNet(nn.Module):
    """Categorical embeddings (+ row dropout) ++ BatchNorm1d'ed, dropped-out continuous inputs -> FullyConnectedNet
    (StructuredData.py:979-1084).  Same constructor, sub-module names and layer groups as the reference.
    `inject_masks(row_masks [n_cat, bs], cont_mask [bs, n_cont])` pins the dropout masks (parity tests)."""

    nnl_default_graphs = True        # launch-bound at notebook batch sizes: Learner replays the whole step as a hipGraph by default

    def __init__(self, target_type, n_cat, n_cont, category_labels, fc_layer_sizes,
                 emb_sizes='default', output_range=None, dropout_levels=None):
        super().__init__()
        self.n_cat, self.n_cont = n_cat, n_cont
        if dropout_levels is None:
            dropout_levels = (0, 0, None)
        self.cont_bn = nn.BatchNorm1d(n_cont)
        self.cont_drop = nn.Dropout(dropout_levels[1])
        if emb_sizes == 'default':
            labels = category_labels if target_type == 'cont' else category_labels[0:-1]
            emb_sizes = [(len(D), embedding_dim(len(D))) for D in labels]
        self.embeddings = nn.ModuleList([EmbeddingDrop(c, d, dropout_levels[0], std=1 / d ** 0.5, max_norm=1.5)
                                         for c, d in emb_sizes])
        layer_sizes = [sum(d for c, d in emb_sizes) + n_cont] + fc_layer_sizes
        final_activ = 'sigmoidal' if (target_type == 'cont' and output_range) else None
        fc = FullyConnectedNet(layer_sizes, dropout_levels[2], final_activ, output_range, pre_bn=False)
        self.head = fc if target_type == 'cat' else nn.Sequential(fc, Flatten1d())
        self.layer_groups = [nn.ModuleList([self.embeddings, self.cont_bn, self.cont_drop]), self.head]
        self.param_groups = separate_bn_layers(self.layer_groups)
        self._plan, self._injected = None, None

    def inject_masks(self, row_masks=None, cont_mask=None):
        self._injected = (row_masks, cont_mask)

    def _masks(self, bs, device):
        if self._injected is not None:
            return self._injected
        row_masks = cont_mask = None
        p_emb = self.embeddings[0].drop.p if self.n_cat > 0 else 0
        p_cont = self.cont_drop.p
        want_rows = self.training and p_emb > 0
        want_cont = self.training and p_cont > 0 and self.n_cont > 0
        if want_rows:          # Layers.py:75-76: drop(ones(len(x))) per column
            row_masks = keyed_mask((self.n_cat, bs), p_emb, device, sample_dim=1)       # None unless Learner.use_keyed_dropout()
        if want_cont:
            cont_mask = keyed_mask((bs, self.n_cont), p_cont, device, sample_dim=0)
        need_rows, need_cont = want_rows and row_masks is None, want_cont and cont_mask is None
        if (need_rows or need_cont) and device.type == 'cuda':
            # both masks from one uniform draw + one launch (Bernoulli(keep) / keep each, as nn.Dropout on ones / on the inputs)
            a, b = ops.keep_masks((self.n_cat, bs) if need_rows else None, 1 - p_emb, (bs, self.n_cont) if need_cont else None, 1 - p_cont, device)
            row_masks = a if need_rows else row_masks
            cont_mask = b if need_cont else cont_mask
        else:
            if need_rows:
                row_masks = torch.empty(self.n_cat, bs, device=device).bernoulli_(1 - p_emb).div_(1 - p_emb)
            if need_cont:
                cont_mask = torch.empty(bs, self.n_cont, device=device).bernoulli_(1 - p_cont).div_(1 - p_cont)
        return row_masks, cont_mask

    def forward(self, xcat_batch, xcont_batch):
        bs, dev = len(xcat_batch), xcat_batch.device
        row_masks, cont_mask = self._masks(bs, dev)
        cont = ops.bn_act(self.cont_bn, xcont_batch, relu=False) if self.n_cont > 0 else None
        if self.n_cat > 0:
            weights = [e.emb.weight for e in self.embeddings]
            sync = getattr(self, 'nnl_dp', None)
            if sync is not None and getattr(self, '_nnl_xren_ready', False):
                sync = tuple(sync[:3]) + (self._nnl_xren,)           # all ranks' indices, gathered before the (captured) step
                self._nnl_xren_ready = False
            combined, self._plan = ops.tab_embed_concat(xcat_batch, weights, row_masks, cont, cont_mask,
                                                        self.embeddings[0].emb.max_norm, self._plan, sync=sync)
        else:
            combined = cont if cont_mask is None else cont * cont_mask
        return self.head(combined)

    def nnl_dp_prepare(self, x_batch, arm=True):
        """Data-parallel replay (Learner.use_graphs under distribute()): the renorm sync's all-gather of every rank's looked-up indices
         run EAGERLY on the step's static input, into a static buffer the captured forward reads — the collective stays
        outside the hipGraph.  arm=True (before the capture): the next forward, the one being captured, reads the buffer; arm=False
        (before a replay): the buffer is refreshed for the graph only, and the next forward that runs in Python (an evaluation, a
        ragged eager step) gathers its own batch's indices.  Returns True when the next forward will use the buffer."""
        sync = getattr(self, 'nnl_dp', None)
        if sync is None or self.n_cat == 0 or self.embeddings[0].emb.max_norm is None:
            return False
        xcat = x_batch[0] if isinstance(x_batch, (list, tuple)) else x_batch
        xren = ops._global_lookup_indices(xcat.contiguous().long(), sync[:3])
        buf = getattr(self, '_nnl_xren', None)
        if buf is None or buf.shape != xren.shape or buf.device != xren.device:
            self._nnl_xren = xren.clone()
        else:
            buf.copy_(xren)
        self._nnl_xren_ready = bool(arm)
        return self._nnl_xren_ready

    @classmethod
    def from_dataobj(cls, data, fc_layer_sizes, emb_sizes='default', output_range=None, dropout_levels=None):
        return cls(data.target_type, data.train_ds.n_cat, data.train_ds.n_cont, data.category_labels, fc_layer_sizes,
                   emb_sizes, output_range, dropout_levels)


class StructuredDataEnsembleNet(nn.Module):
    "Weighted average of several tabular models, optional softmax correction (StructuredData.py:1098-1133)"

    def __init__(self, models, weights=None, correction=None):
        super().__init__()
        n = len(models)
        self.weights = weights if weights else [1 / n] * n
        self.correction = correction
        self.models = nn.ModuleList(models)
        self.layer_groups = models
        self.param_groups = separate_bn_layers(self.layer_groups)

    def forward(self, xcat, xcont):
        if self.correction is None:
            return sum(w * m(xcat, xcont) for w, m in zip(self.weights, self.models))
        if self.correction == 'cat':
            return sum(w * F.log_softmax(m(xcat, xcont), dim=1).exp() for w, m in zip(self.weights, self.models))
