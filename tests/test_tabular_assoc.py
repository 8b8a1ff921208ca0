"""EDA association measures (Applications/StructuredData.py §1.2) against G22 (tests/golden/g22_tabular_assoc.npz: the real reference on
the frame tools/gen_golden_tabular_assoc.py builds, next to an np.longdouble restatement of every value), and the HIP entries behind
them (nnl_assoc_contingency, nnl_assoc_table_stats, nnl_assoc_cat_cont, nnl_assoc_cont_cont, K13) against numpy over their tile,
route and chunk boundaries.

Tolerances (u = 2^-53, the unit roundoff of fp64).
Counts are integers: exact.  n, the numbers of non-empty rows / columns / categories, min and max: exact.
Moment-based measures (correlation_ratio, max_correlation_ratio, abs_correlation, abs_max_correlation) against the restatement:
every sum the kernels take has n terms that are added in some tree or sequence of fp64 additions, so its relative error is at most
about n u against the sum of the terms' magnitudes; the sums are centred (about the column's nanmean, then about the pair's mean), so
for the fixtures here that sum of magnitudes is within a small factor of the sum itself.  A correlation is a ratio
S_ab / sqrt(S_aa S_bb) with |S_ab| <= sqrt(S_aa S_bb) (Cauchy-Schwarz), so relative errors e in the three sums move it by at most
about 2 e in absolute terms; the ratios of the correlation-ratio family are square roots of such quotients.  With the products, the
one-pass variance identity and the final division and square root this stays below 16 n u, taken as both the absolute and the
relative tolerance.
Entropy-based measures (mutual_info_*) against the restatement: H_X, H_Y and H_XY are sums of at most `cells` terms -p log p, each
computed to a few u and added in fp64: an absolute error of at most about cells u H each.  I = H_X + H_Y - H_XY then carries
cells u (H_X + H_Y + H_XY) and the normed value divides by H_X or H_Y: 16 cells u (H_X + H_Y + H_XY) / min(H_X, H_Y), from the
restatement's own terms (stored per pair in G22).  The direct entropy helpers: 16 cells u max(H, 1).
Against the reference: the bound above plus the distance d_<Type> the generator recorded between the reference and the restatement.
Short-circuit cases (X == Y, no common row, a single distinct value): exactly 1.0 / 0.0."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from tools.gen_golden_tabular_assoc import (CAT_VARS, CONT_VARS, DEPENDENT, DIRECT, TYPES, cat_cont_exact, cat_terms, cont_exact, frame,
                                            pairs_of)

from neuralnetworklibrary_amd import ops
from neuralnetworklibrary_amd._lib import NnlError, lib
from neuralnetworklibrary_amd.Applications import StructuredData as SD

DEV = 'cuda'
U = 2.0 ** -53
T = ops.ASSOC_ROW_TILE
ROW_COUNTS = [1, 2, T - 1, T, T + 1, 2 * T + 3]
MANY_TILES = (ops.ASSOC_MAX_GROUPS + 1) * T + 3          # the one size at which a workgroup owns more than one tile


@pytest.fixture(scope='module')
def g22():
    return load_golden('g22_tabular_assoc')


@pytest.fixture(scope='module')
def df():
    return frame()


def same(a, b):
    a, b = np.asarray(a, dtype='float64'), np.asarray(b, dtype='float64')
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def moment_tol(n):
    "16 n u; below 16 rows the ten or so roundings of the closing formula (products, the division, the square root) outweigh the sums'"
    return 16 * max(n, 16) * U


def entropy_tol(terms):
    "terms [..., 4] = H_X, H_Y, H_XY, cells of the restatement -> the bound on a normed mutual information (NaN where short-circuited)"
    hx, hy, hxy, cells = np.moveaxis(np.asarray(terms, dtype='float64'), -1, 0)
    return 16 * cells * U * (hx + hy + hxy) / np.minimum(hx, hy)


def check_values(got, ref, exact, tol, d):
    "tol: scalar or array (NaN where the pair is short-circuited: there the value is exact)"
    got, ref, exact = [np.asarray(a, dtype='float64') for a in (got, ref, exact)]
    tol = np.broadcast_to(np.asarray(tol, dtype='float64'), exact.shape)
    short = (exact == 0.0) | (exact == 1.0)
    assert np.array_equal(got[short], exact[short]), 'short-circuit cases must be exactly 1.0 / 0.0'
    assert short.sum() < short.size
    err_e, err_r = np.abs(got - exact)[~short], np.abs(got - ref)[~short]
    bound = tol[~short] * np.maximum(1.0, np.abs(exact[~short]))
    print('max error vs restatement %.3e, vs reference %.3e, smallest bound %.3e, d %.3e' % (err_e.max(), err_r.max(), bound.min(), d))
    assert np.isfinite(bound).all()
    assert (err_e <= bound).all() and (err_r <= bound + d).all()


# ---- no GPU --------------------------------------------------------------------------------------------------------------

def test_generator_frame_is_the_one_g22_was_made_from(g22, df):
    assert np.array_equal(g22['in.index'], df.index) and g22['in.columns'].tolist() == list(df.columns)
    assert list(df.columns) == CAT_VARS + CONT_VARS
    for c in df.columns:
        want = g22['in.col.' + c]
        assert np.array_equal(want, df[c].astype(str).to_numpy(dtype='U')) if df[c].dtype == object else same(want, df[c])


def test_missing_value_counts_matches_the_reference(g22, df):
    got = SD.missing_value_counts(df)
    assert list(got.index) == g22['missing.index'].tolist() and np.array_equal(got.to_numpy(), g22['missing.values'])
    assert len(SD.missing_value_counts(df[['s4', 'skew']])) == 0


def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_abi_entries_validate_before_any_hip_call():
    "null pointers, n outside [1, 2^31), P < 1 and a pair index outside [0, V): -1 and the entry's own name, without a GPU"
    fake = ctypes.c_void_p(4096)                 # stands for a device pointer: validation never follows it
    _c, card = _host([2, 3], np.int32)
    _g, good = _host([0], np.int32)
    _b, bad = _host([2], np.int32)
    _n, neg = _host([-1], np.int32)
    _1, one = _host([1], np.int32)
    _o, off = _host([0, 6], np.int64)            # the pair (0, 1): 2 x 3 cells
    _s, short = _host([0, 5], np.int64)
    n_ok = 5

    def contingency(codes=fake, card=card, n=n_ok, px=good, py=one, off=off, P=1, tables=fake):
        return lib.nnl_assoc_contingency(codes, card, 2, n, px, py, off, P, tables, None)

    def stats(tables=fake, px=good, py=one, P=1, out=fake):
        return lib.nnl_assoc_table_stats(tables, card, 2, px, py, off, P, out, None)

    def cat_cont(codes=fake, n=n_ok, px=good, py=good, P=1, ws=fake, out=fake):
        return lib.nnl_assoc_cat_cont(codes, card, 2, fake, fake, 2, n, px, py, P, ws, 1 << 20, out, None)

    def cont_cont(vals=fake, n=n_ok, px=good, py=good, P=1, with_abs=1, out=fake):
        return lib.nnl_assoc_cont_cont(vals, fake, 2, n, px, py, P, with_abs, fake, 1 << 20, out, None)
    cases = {
        b'assoc_contingency': [contingency(codes=None), contingency(tables=None), contingency(n=0), contingency(n=2 ** 31), contingency(P=0),
                               contingency(px=bad), contingency(py=neg), contingency(off=short)],
        b'assoc_table_stats': [stats(tables=None), stats(out=None), stats(P=0), stats(px=neg), stats(py=bad)],
        b'assoc_cat_cont': [cat_cont(codes=None), cat_cont(out=None), cat_cont(n=0), cat_cont(n=2 ** 31), cat_cont(P=0), cat_cont(px=bad),
                            cat_cont(py=neg)],
        b'assoc_cont_cont': [cont_cont(vals=None), cont_cont(out=None), cont_cont(n=0), cont_cont(n=2 ** 31), cont_cont(P=0),
                             cont_cont(px=bad), cont_cont(py=neg), cont_cont(with_abs=2)],
    }
    for name, statuses in cases.items():
        assert statuses == [-1] * len(statuses), (name, statuses)
    for name, call in ((b'assoc_contingency', contingency), (b'assoc_table_stats', stats), (b'assoc_cat_cont', cat_cont),
                       (b'assoc_cont_cont', cont_cont)):
        assert call(px=bad) == -1 and name in lib.nnl_last_error()
    assert lib.nnl_assoc_cat_cont_workspace_bytes(card, 2, good, 1) == 8 * (3 * 2 + 2)
    assert lib.nnl_assoc_cat_cont_workspace_bytes(card, 2, bad, 1) == 0 and lib.nnl_assoc_cont_cont_workspace_bytes(0, 1) == 0
    # a workspace that is too small is refused as well
    assert lib.nnl_assoc_cont_cont(fake, fake, 2, n_ok, good, good, 1, 1, fake, 8, fake, None) == -1 and b'workspace' in lib.nnl_last_error()


def test_ops_refuse_cpu_tensors():
    codes, vals, shift = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    with pytest.raises(NnlError):
        ops.assoc_contingency(codes, [2, 2], [0], [1])
    with pytest.raises(NnlError):
        ops.assoc_table_stats(torch.zeros(4, dtype=torch.int32), [2, 2], [0], [1], [0, 4])
    with pytest.raises(NnlError):
        ops.assoc_cat_cont(codes, [2, 2], vals, shift, [0], [1])
    with pytest.raises(NnlError):
        ops.assoc_cont_cont(vals, shift, [0], [1])


def test_helpers_raise_on_missing_and_infinite_values(df):
    "before anything is uploaded: these raise without a GPU"
    for call, column in ((lambda: SD.entropy(df, 'fcode'), 'fcode'), (lambda: SD.joint_entropy(df, 's4', 'fcode'), 'fcode'),
                         (lambda: SD.normed_mutual_info(df, 'fcode', 's4', True), 'fcode'), (lambda: SD.correlation_ratio(df, 's4', 'xn'), 'xn'),
                         (lambda: SD.max_correlation_ratio(df, 'fcode', 'skew'), 'fcode'), (lambda: SD.abs_max_correlation(df, 'xn', 'skew'), 'xn')):
        with pytest.raises(ValueError, match=column):
            call()
    bad = df.copy()
    bad.loc[bad.index[3], 'skew'] = -np.inf
    for call in (lambda: SD.abs_max_correlation(bad, 'skew', 'ival'), lambda: SD.get_association(bad, 's4', 'skew', 'correlation_ratio'),
                 lambda: SD.associations_pairs(bad, 'abs_correlation', cont_vars=['xn', 'skew'], plot=False)):
        with pytest.raises(ValueError, match='skew'):
            call()
    with pytest.raises(ValueError, match='Type'):
        SD.get_association(df, 's4', 'skew', 'pearson')


# ---- the public API against G22 ------------------------------------------------------------------------------------------

def _tolerance(g22, key, Type, n):
    return entropy_tol(g22[key + '_terms']) if TYPES[Type] == 'cat' else moment_tol(n)


@pytest.mark.gpu
@pytest.mark.parametrize('Type', list(TYPES))
def test_associations_pairs_match_g22(g22, df, Type):
    rows, cols, cat_vars, cont_vars = pairs_of(Type)
    before = df.copy()
    got = SD.associations_pairs(df, Type, cat_vars=cat_vars, cont_vars=cont_vars, plot=False)
    assert isinstance(got, pd.DataFrame) and list(got.index) == rows and list(got.columns) == cols
    assert all(t == np.float64 for t in got.dtypes)
    assert df.equals(before) and list(df.dtypes) == list(before.dtypes) and df.index.equals(before.index)
    key = 'pairs.' + Type
    check_values(got.to_numpy(), g22[key], g22[key + '_exact'], _tolerance(g22, key, Type, len(df)), float(g22['d_' + Type]))
    # a single get_association is the same path with one pair
    i, j = (1, 2) if TYPES[Type] != 'cat_cont' else (1, 0)
    one = SD.get_association(df, rows[i], cols[j], Type)
    assert isinstance(one, float) and one == got.iloc[i, j] or TYPES[Type] == 'cat_cont' and abs(one - got.iloc[i, j]) <= moment_tol(len(df))
    assert SD.get_association(df, rows[0], rows[0], Type) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('k', range(len(DEPENDENT)))
def test_associations_dependent_match_g22(g22, df, k):
    Type, variables, depend_var, reverse = DEPENDENT[k]
    before = df.copy()
    got = SD.associations_dependent(df, Type, variables, depend_var, reverse=reverse, plot=False)
    assert isinstance(got, pd.Series) and list(got.index) == variables and got.dtype == np.float64
    assert df.equals(before)
    key = 'dependent.%d' % k
    check_values(got.to_numpy(), g22[key], g22[key + '_exact'], _tolerance(g22, key, Type, len(df)), float(g22['d_' + Type]))


@pytest.mark.gpu
def test_direct_helpers_match_g22(g22, df):
    before = df.copy()
    for k, (name, args) in enumerate(DIRECT):
        got = getattr(SD, name)(df, *args)
        ref, exact = float(g22['direct.%d' % k]), float(g22['direct.%d_exact' % k])
        if name in ('entropy', 'joint_entropy', 'normed_mutual_info'):
            hx, hy, hxy, cells = [float(v) for v in cat_terms(df, args[0], args[1] if len(args) > 1 else args[0])]
            tol = {'entropy': 16 * df[args[0]].nunique() * U * max(hx, 1.0), 'joint_entropy': 16 * cells * U * max(hxy, 1.0),
                   'normed_mutual_info': float(entropy_tol([hx, hy, hxy, cells]))}[name]
        else:
            tol = moment_tol(len(df)) * max(1.0, abs(exact))
        print(name, args, 'got %.17g exact %.17g ref %.17g tol %.3e' % (got, exact, ref, tol))
        assert isinstance(got, float) and abs(got - exact) <= tol and abs(got - ref) <= tol + abs(ref - exact)
    assert df.equals(before)


@pytest.mark.gpu
def test_plot_needs_its_libraries_and_says_which(df):
    try:
        import seaborn  # noqa: F401
        import matplotlib  # noqa: F401
    except ImportError as e:
        with pytest.raises(ImportError, match=e.name):
            SD.associations_pairs(df, 'abs_correlation', cont_vars=['xn', 'skew'], plot=True)
        return
    import matplotlib
    matplotlib.use('Agg')
    got = SD.associations_pairs(df, 'abs_correlation', cont_vars=['xn', 'skew'], plot=True)
    assert got.shape == (2, 2)


# ---- the kernels against numpy -------------------------------------------------------------------------------------------

def routes(fn):
    lib.nnl_debug_route_record(1)
    try:
        out = fn()
        buf = ctypes.create_string_buffer(4096)
        assert lib.nnl_debug_route_collect(buf, len(buf)) >= 0
    finally:
        lib.nnl_debug_route_record(0)
    return out, buf.value.decode()


def make_codes(rs, n, cards, missing=0.1):
    "int32 [V, n]: every column uniform over its categories with `missing` of -1, and -1 in the first and last row of every tile"
    codes = np.stack([rs.randint(0, c, n) for c in cards]).astype(np.int32)
    codes[rs.random_sample(codes.shape) < missing] = -1
    if n > 2:
        for edge in list(range(0, n, T)) + list(range(T - 1, n, T)):
            codes[edge % len(cards), edge] = -1
    return codes


def tables_numpy(codes, card, px, py):
    out = []
    for x, y in zip(px, py):
        ok = (codes[x] >= 0) & (codes[y] >= 0)
        out.append(np.bincount(codes[x][ok].astype(np.int64) * card[y] + codes[y][ok], minlength=card[x] * card[y]))
    return np.concatenate(out)


def stats_numpy(table, cx, cy):
    "n, rows, cols, H_X, H_Y, H_XY in longdouble (the clamp term included)"
    t = table.reshape(cx, cy).astype(np.longdouble)
    n = t.sum()
    if n == 0:
        return [0.0] * 6

    def h(c):
        p = c[c > 0] / n
        return -(np.log(p) * p).sum()
    r, c = t.sum(1), t.sum(0)
    empty = int((r > 0).sum()) * int((c > 0).sum()) - int((t > 0).sum())
    return [float(v) for v in (n, (r > 0).sum(), (c > 0).sum(), h(r), h(c), h(t.ravel()) + empty * -(np.longdouble(1e-20) * np.log(np.longdouble(1e-20))))]


def run_contingency(codes, card, px, py):
    d = torch.from_numpy(codes).to(DEV)
    (tables, offsets), route = routes(lambda: ops.assoc_contingency(d, card, px, py))
    want = tables_numpy(codes, card, px, py)
    got = tables.cpu().numpy()
    assert np.array_equal(offsets, ops.assoc_table_offsets(card, px, py)) and got.shape == want.shape
    assert np.array_equal(got, want), 'counts differ: they must be exact'
    st = ops.assoc_table_stats(tables, card, px, py, offsets)
    again_t, _ = ops.assoc_contingency(d, card, px, py)
    again = ops.assoc_table_stats(again_t, card, px, py, offsets)
    assert torch.equal(again_t, tables) and torch.equal(st, again), 'counts and table statistics must be bit-equal from call to call'
    st = st.cpu().numpy()
    for p, (x, y) in enumerate(zip(px, py)):
        w = stats_numpy(want[offsets[p]:offsets[p + 1]], card[x], card[y])
        assert np.array_equal(st[p, :3], w[:3]), (p, st[p], w)
        cells = card[x] * card[y]
        np.testing.assert_allclose(st[p, 3:], w[3:], rtol=0, atol=16 * cells * U * max(1.0, w[5]))
    return route


@pytest.mark.gpu
@pytest.mark.parametrize('n', ROW_COUNTS + [MANY_TILES])
def test_contingency_counts_are_exact_at_tile_edges(n):
    "cardinalities 1 and 2 among them, an all-missing column (3), a pair with no common row (4, 5), one pair and many"
    rs = np.random.RandomState(n)
    card = [1, 2, 7, 5, 3, 4, 300, 31, 12, 9]
    codes = make_codes(rs, n, card)
    codes[3] = -1
    half = np.arange(n) % 2 == 0
    codes[4][half], codes[5][~half] = -1, -1
    route = run_contingency(codes, card, [2], [7])
    assert 'assoc_contingency:lds=1,global=0,chunks=1' in route
    V = len(card)
    px, py = [i for i in range(V) for j in range(V)], [j for i in range(V) for j in range(V)]      # 100 pairs over 10 columns
    assert len(px) > ops.ASSOC_CONTINGENCY_PAIRS
    route = run_contingency(codes, card, px, py)
    n_global = sum(card[x] * card[y] > ops.ASSOC_LDS_CELLS for x, y in zip(px, py))
    assert n_global == 3                                                    # 300 x 300, 300 x 31 and 31 x 300
    assert 'lds=%d,global=%d' % (len(px) - n_global, n_global) in route and 'chunks=1;' not in route


@pytest.mark.gpu
def test_contingency_route_changes_at_the_lds_limit():
    rs = np.random.RandomState(7)
    n = 2 * T + 3
    assert 96 * 64 == ops.ASSOC_LDS_CELLS
    card = [96, 64, 97]
    codes = make_codes(rs, n, card)
    below = run_contingency(codes, card, [0], [1])
    above = run_contingency(codes, card, [2], [1])
    assert 'lds=1,global=0' in below and 'lds=0,global=1' in above and below != above
    both = run_contingency(codes, card, [0, 2, 1], [1, 1, 0])
    assert 'lds=2,global=1' in both


@pytest.mark.gpu
def test_limits_raise_value_error():
    codes = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='cells'):
        ops.assoc_contingency(codes, [8193, 8193], [0], [1])
    assert 4096 * 4096 <= ops.ASSOC_MAX_TABLE_CELLS
    with pytest.raises(ValueError, match='outside'):
        ops.assoc_contingency(codes, [2, 2], [0], [2])
    with pytest.raises(ValueError, match='outside'):
        ops.assoc_cont_cont(codes.double(), torch.zeros(2, dtype=torch.float64, device=DEV), [0], [-1])


def make_vals(rs, n, V):
    "float64 [V, n]: columns of different location and scale with NaNs; column 1 is all NaN, 2 a constant, 3 / 4 complementary"
    vals = rs.standard_normal((V, n)) * (1 + np.arange(V))[:, None] + 10 * np.arange(V)[:, None]
    vals[rs.random_sample(vals.shape) < 0.1] = np.nan
    vals[1] = np.nan
    vals[2] = 3.5
    half = np.arange(n) % 2 == 0
    vals[3][half], vals[4][~half] = np.nan, np.nan
    if n > 2:
        vals[5, 0] = vals[5, n - 1] = np.nan
    return vals


def shifts_of(vals):
    return np.array([np.nanmean(v) if not np.isnan(v).all() else 0.0 for v in vals])


@pytest.mark.gpu
@pytest.mark.parametrize('n', ROW_COUNTS + [MANY_TILES])
def test_cat_cont_moments_match_longdouble(n):
    rs = np.random.RandomState(100 + n)
    card = [1, 2, 7, 5, ops.ASSOC_MOMENT_LDS_CELLS, ops.ASSOC_MOMENT_LDS_CELLS + 1]
    codes, vals = make_codes(rs, n, card), make_vals(rs, n, 6)
    codes[3] = -1
    shift = shifts_of(vals)
    px, py = [i for i in range(6) for j in range(6)], [j for i in range(6) for j in range(6)]
    d_codes, d_vals, d_shift = [torch.from_numpy(a).to(DEV) for a in (codes, vals, shift)]
    out, route = routes(lambda: ops.assoc_cat_cont(d_codes, card, d_vals, d_shift, px, py))
    assert 'assoc_cat_cont:lds=30,global=6' in route               # the card above the LDS limit takes global atomics
    one = ops.assoc_cat_cont(d_codes, card, d_vals, d_shift, [2], [0]).cpu().numpy()
    out = out.cpu().numpy()
    np.testing.assert_allclose(one[0], out[2 * 6 + 0], rtol=moment_tol(n), atol=0)
    assert np.array_equal(one[0, [0, 1, 4, 5]], out[2 * 6, [0, 1, 4, 5]])
    for p, (x, y) in enumerate(zip(px, py)):
        ok = (codes[x] >= 0) & ~np.isnan(vals[y])
        assert out[p, 0] == ok.sum()
        if not ok.any():
            assert np.array_equal(out[p], np.zeros(6))
            continue
        assert out[p, 1] == len(np.unique(codes[x][ok]))
        ys = vals[y][ok] - shift[y]
        assert out[p, 4] == ys.min() and out[p, 5] == ys.max()
        if out[p, 1] > 1 and ys.min() < ys.max():
            D = pd.DataFrame({'x': codes[x][ok], 'y': vals[y][ok]})
            ratio, raw = [float(v) for v in cat_cont_exact(D, 'x', 'y')]
            tol = moment_tol(ok.sum())
            assert abs(out[p, 2] - ratio) <= tol * max(1.0, ratio) and abs(out[p, 3] - raw) <= tol * max(1.0, raw), (p, out[p], ratio, raw)


@pytest.mark.gpu
@pytest.mark.parametrize('n', ROW_COUNTS + [MANY_TILES])
def test_cont_cont_correlations_match_longdouble_and_repeat(n):
    rs = np.random.RandomState(200 + n)
    V = 7
    vals = make_vals(rs, n, V)
    vals[6] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 if n % 2 == 0 else 1.5)       # balanced +-1 for even n
    shift = shifts_of(vals)
    px, py = [i for i in range(V) for j in range(V)], [j for i in range(V) for j in range(V)]
    assert len(px) > ops.ASSOC_CONT_PAIRS
    d_vals, d_shift = torch.from_numpy(vals).to(DEV), torch.from_numpy(shift).to(DEV)
    out, route = routes(lambda: ops.assoc_cont_cont(d_vals, d_shift, px, py, with_abs=True))
    assert 'assoc_cont_cont:two-pass' in route
    again = ops.assoc_cont_cont(d_vals, d_shift, px, py, with_abs=True)
    assert torch.equal(out.view(torch.int64), again.view(torch.int64)), 'no atomics: bit-equal from call to call'
    first, route = routes(lambda: ops.assoc_cont_cont(d_vals, d_shift, px, py, with_abs=False))
    assert 'assoc_cont_cont:one-pass' in route
    out, first = out.cpu().numpy(), first.cpu().numpy()
    assert same(first[:, :3], out[:, :3]) and np.isnan(first[:, 3]).all()
    one = ops.assoc_cont_cont(d_vals, d_shift, [0], [5]).cpu().numpy()
    assert n < 3 or not np.isnan(one[0, 3])
    np.testing.assert_allclose(one[0], out[5], rtol=moment_tol(n), atol=0)
    for p, (x, y) in enumerate(zip(px, py)):
        ok = ~np.isnan(vals[x]) & ~np.isnan(vals[y])
        xs, ys = vals[x][ok], vals[y][ok]
        degenerate = not ok.any() or xs.min() == xs.max() or ys.min() == ys.max()
        assert out[p, 0] == ok.sum() and out[p, 1] == float(degenerate)
        if degenerate:
            assert np.isnan(out[p, 2:]).all()
            continue
        c1, best = [float(v) for v in cont_exact(pd.DataFrame({'x': xs, 'y': ys}), 'x', 'y')]
        tol = moment_tol(ok.sum())
        assert abs(out[p, 2] - c1) <= tol and abs(out[p, 3] - best) <= tol, (p, x, y, out[p], c1, best)
