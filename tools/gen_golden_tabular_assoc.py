"""Golden vectors G22 for the EDA association measures (reference Applications/StructuredData.py:235-428: missing_value_counts, entropy,
joint_entropy, normed_mutual_info, correlation_ratio, max_correlation_ratio, abs_max_correlation, get_association,
associations_dependent, associations_pairs).

Runs the REAL reference on CPU through oracle/_ref_import.py (read-only) and writes arrays only (loadable with allow_pickle=False) to
tests/golden/g22_tabular_assoc.npz.  The frame is built here by `frame()` from seeded np.random.RandomState draws; the tests rebuild it
with the same function and G22 stores its columns as a cross-check.

The frame, 600 rows.  Categorical: 's4' a string column with 4 values; 'fcode' float-coded integers (values >= 10) with NaNs;
'c300' 300 values; 'bin' binary; 'one' a single value.  Continuous: 'xn' normal with NaNs; 'skew' exponential whose mean depends on
's4'; 'ival' integer-valued; 'const' a constant; 'allnan'; 'pm1' balanced +-1 (|pm1 - mean| is exactly constant on the NaN-free
rows); 'ca' / 'cb' whose NaN rows are complementary (the pair has no common row).

Stored: associations_pairs for all six Types in their modes (cat x cat, cat x cont, cont x cont), associations_dependent with reverse
both ways, the six direct helpers on NaN-free columns, missing_value_counts.  Next to every reference value stands an np.longdouble
restatement from the definitions (`*_exact`), and per Type the largest distance between the two (`d_<Type>`).  For the entropy-based
Types `*_terms` holds the restatement's H_X, H_Y, H_XY and the number of cells of the observed table per pair (NaN where the pair is
short-circuited), from which the tests derive their bound.

Asserted here, because the tests rely on it: no |X - mean(X)| of any cont x cont pair has a centred sum of squares between
n (2^-40 mean)^2 and n (2^-12 mean)^2 (the constancy rule of abs_max_correlation stays away from every fixture but 'pm1'); the
reference returns a finite value in [0, 1] for every stored pair.
Usage: python tools/gen_golden_tabular_assoc.py   (needs the reference checkout the oracle shim points at)"""
import os
import sys
import warnings

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g22_tabular_assoc.npz')
N_ROWS = 600
CAT_VARS = ['s4', 'fcode', 'c300', 'bin', 'one']
CONT_VARS = ['xn', 'skew', 'ival', 'const', 'allnan', 'pm1', 'ca', 'cb']
TYPES = {'mutual_info_symmetric': 'cat', 'mutual_info_asymmetric': 'cat', 'correlation_ratio': 'cat_cont',
         'max_correlation_ratio': 'cat_cont', 'abs_correlation': 'cont', 'abs_max_correlation': 'cont'}
# (Type, variables, depend_var, reverse)
DEPENDENT = [('correlation_ratio', CAT_VARS, 'skew', False), ('max_correlation_ratio', CONT_VARS, 's4', True),
             ('mutual_info_asymmetric', CAT_VARS, 'bin', False), ('mutual_info_asymmetric', CAT_VARS, 'bin', True),
             ('abs_max_correlation', CONT_VARS, 'skew', False)]
# the six direct helpers, on NaN-free columns: (name, arguments)
DIRECT = [('entropy', ('s4',)), ('entropy', ('c300',)), ('joint_entropy', ('s4', 'bin')), ('joint_entropy', ('c300', 's4')),
          ('normed_mutual_info', ('s4', 'c300', True)), ('normed_mutual_info', ('s4', 'c300', False)),
          ('correlation_ratio', ('s4', 'skew')), ('correlation_ratio', ('c300', 'ival')), ('max_correlation_ratio', ('c300', 'skew')),
          ('abs_max_correlation', ('skew', 'ival')), ('abs_max_correlation', ('pm1', 'skew'))]
LD = np.longdouble


def frame():
    "600 rows: the columns of CAT_VARS and CONT_VARS (see the module docstring), on an index that is not 0 .. n-1"
    rs = np.random.RandomState(2201)
    n = N_ROWS
    s4 = rs.choice(['north', 'south', 'east', 'west'], n, p=[.4, .3, .2, .1]).astype(object)
    fcode = rs.choice([10., 11., 23., 100., 7.], n)
    fcode[rs.choice(n, 40, replace=False)] = np.nan
    c300 = rs.randint(0, 300, n)
    level = pd.Series(s4).map({'north': 1.0, 'south': 2.0, 'east': 4.0, 'west': 8.0}).to_numpy()
    xn = rs.standard_normal(n) * 2.5 + 10
    xn[rs.choice(n, 50, replace=False)] = np.nan
    pm1 = np.repeat([1.0, -1.0], n // 2)[rs.permutation(n)]
    ca, cb = rs.standard_normal(n), rs.standard_normal(n)
    half = rs.permutation(n) < n // 2
    ca[half], cb[~half] = np.nan, np.nan
    df = pd.DataFrame({'s4': s4, 'fcode': fcode, 'c300': c300, 'bin': (rs.random_sample(n) < .3).astype('int64'), 'one': 'only',
                       'xn': xn, 'skew': rs.exponential(level), 'ival': rs.randint(-5, 40, n).astype('float64') + 3 * (c300 % 3),
                       'const': 4.25, 'allnan': np.nan, 'pm1': pm1, 'ca': ca, 'cb': cb})
    df.index = df.index + 5000
    return df


def pair_rows(df, X, Y):
    return df[df[X].notnull() & df[Y].notnull()]


def _entropy_ld(counts):
    p = counts[counts > 0].astype(LD) / LD(counts.sum())
    return -(np.log(p) * p).sum(dtype=LD)


def cat_terms(D, X, Y):
    "H_X, H_Y, H_XY (with the clamp term) and the cells of the observed table, in longdouble"
    cx, cy = pd.factorize(D[X])[0], pd.factorize(D[Y])[0]
    kx, ky = cx.max() + 1, cy.max() + 1
    table = np.bincount(cx * ky + cy, minlength=kx * ky)
    hxy = _entropy_ld(table) + LD(int((table == 0).sum())) * -(LD(1e-20) * np.log(LD(1e-20)))
    return _entropy_ld(np.bincount(cx)), _entropy_ld(np.bincount(cy)), hxy, kx * ky


def cat_cont_exact(D, X, Y):
    "(correlation ratio, raw max ratio) in longdouble"
    codes = pd.factorize(D[X])[0]
    y = D[Y].to_numpy(dtype='float64').astype(LD)
    n = LD(len(y))
    mean = y.sum(dtype=LD) / n
    var = ((y - mean) ** 2).sum(dtype=LD) / (n - 1)
    between, dev = LD(0), LD(0)
    for k in range(codes.max() + 1):
        yk = y[codes == k]
        d = yk.sum(dtype=LD) / LD(len(yk)) - mean
        between += LD(len(yk)) * d * d
        dev = max(dev, abs(d))
    return np.sqrt(between / n / var), dev / np.sqrt(var)


def _centred(v):
    return v - v.sum(dtype=LD) / LD(len(v))


def x2_spread(v):
    "(centred sum of squares of |v - mean|, n mean(|v - mean|)^2) in longdouble"
    a = np.abs(_centred(v.astype(LD)))
    return (_centred(a) ** 2).sum(dtype=LD), LD(len(a)) * (a.sum(dtype=LD) / LD(len(a))) ** 2


def cont_exact(D, X, Y):
    "(|c1|, abs max correlation) in longdouble; a correlation with an exactly constant |v - mean| is skipped"
    x, y = D[X].to_numpy(dtype='float64').astype(LD), D[Y].to_numpy(dtype='float64').astype(LD)
    dx, dy = _centred(x), _centred(y)
    const_x2, const_y2 = [s <= 2.0 ** -80 * m for s, m in (x2_spread(x), x2_spread(y))]

    def corr(a, b):
        return abs((a * b).sum(dtype=LD) / np.sqrt((a * a).sum(dtype=LD) * (b * b).sum(dtype=LD)))
    c1 = corr(dx, dy)
    cs = [c1]
    if not const_y2:
        cs.append(corr(dx, _centred(np.abs(dy))))
    if not const_x2:
        cs.append(corr(_centred(np.abs(dx)), dy))
    if not const_x2 and not const_y2:
        cs.append(corr(_centred(np.abs(dx)), _centred(np.abs(dy))))
    return c1, max(cs)


def association_exact(df, X, Y, Type):
    "get_association from the definitions in longdouble -> (value, terms or None)"
    if X == Y:
        return 1.0, None
    D = pair_rows(df, X, Y)
    if len(D) == 0 or D[X].nunique() == 1 or D[Y].nunique() == 1:
        return 0.0, None
    if TYPES[Type] == 'cat':
        hx, hy, hxy, cells = cat_terms(D, X, Y)
        i_xy = hx + hy - hxy
        v = i_xy / hy if Type == 'mutual_info_asymmetric' else LD(0.5) * (i_xy / hx + i_xy / hy)
        return float(v), (float(hx), float(hy), float(hxy), float(cells))
    if TYPES[Type] == 'cat_cont':
        ratio, raw = cat_cont_exact(D, X, Y)
        return float(ratio if Type == 'correlation_ratio' else min(raw / 3, LD(1))), None
    c1, best = cont_exact(D, X, Y)
    return float(c1 if Type == 'abs_correlation' else best), None


def direct_exact(df, name, args):
    if name == 'entropy':
        return float(_entropy_ld(np.bincount(pd.factorize(df[args[0]])[0])))
    if name == 'joint_entropy':
        return float(cat_terms(df, *args)[2])
    if name == 'normed_mutual_info':
        hx, hy, hxy, _ = cat_terms(df, args[0], args[1])
        i_xy = hx + hy - hxy
        return float(LD(0.5) * (i_xy / hx + i_xy / hy) if args[2] else i_xy / hy)
    if name == 'correlation_ratio':
        return float(cat_cont_exact(df, *args)[0])
    if name == 'max_correlation_ratio':
        return float(cat_cont_exact(df, *args)[1])
    return float(cont_exact(df, *args)[1])


def pairs_of(Type):
    "(rows, columns, cat_vars, cont_vars) of the associations_pairs call stored for Type"
    mode = TYPES[Type]
    if mode == 'cat':
        return CAT_VARS, CAT_VARS, CAT_VARS, None
    if mode == 'cont':
        return CONT_VARS, CONT_VARS, None, CONT_VARS
    return CAT_VARS, CONT_VARS, CAT_VARS, CONT_VARS


def check_spread(df):
    for X in CONT_VARS:
        for Y in CONT_VARS:
            D = pair_rows(df, X, Y)
            if X == Y or len(D) == 0 or D[X].nunique() == 1 or D[Y].nunique() == 1:
                continue
            for v in (X, Y):
                ss, nm2 = x2_spread(D[v].to_numpy(dtype='float64'))
                assert not (2.0 ** -80 * nm2 < ss < 2.0 ** -24 * nm2), (X, Y, v, float(ss), float(nm2))
                if ss <= 2.0 ** -80 * nm2:
                    assert v == 'pm1', (X, Y, v)


def main():
    from oracle import _ref_import
    SD = _ref_import.load()['Applications.StructuredData']
    SD.PBar = lambda it, *a, **k: it
    warnings.simplefilter('ignore')
    df = frame()
    before = df.copy()
    check_spread(df)
    out = {'in.index': np.asarray(df.index), 'in.columns': np.array(list(df.columns))}
    for c in df.columns:
        out['in.col.' + c] = df[c].astype(str).to_numpy(dtype='U') if df[c].dtype == object else df[c].to_numpy()
    mv = SD.missing_value_counts(df)
    out['missing.index'], out['missing.values'] = np.array(list(mv.index)), mv.to_numpy().astype('int64')

    for Type in TYPES:
        rows, cols, cat_vars, cont_vars = pairs_of(Type)
        ref = SD.associations_pairs(df, Type, cat_vars=cat_vars, cont_vars=cont_vars, plot=False)
        assert list(ref.index) == rows and list(ref.columns) == cols
        r = ref.to_numpy(dtype='float64')
        assert np.isfinite(r).all() and (r >= 0).all() and (r <= 1).all(), (Type, r)
        exact, terms = np.zeros_like(r), np.full(r.shape + (4,), np.nan)
        for i, X in enumerate(rows):
            for j, Y in enumerate(cols):
                exact[i, j], t = association_exact(df, X, Y, Type)
                if t is not None:
                    terms[i, j] = t
        short = (exact == 0.0) | (exact == 1.0)
        assert np.array_equal(r[short], exact[short]), (Type, 'short-circuit values')
        d = float(np.abs(r - exact).max())
        print('%-24s %s d %.3e, %d of %d pairs short-circuited' % (Type, r.shape, d, short.sum(), short.size), flush=True)
        assert d < 1e-9, (Type, d)
        out['pairs.%s' % Type], out['pairs.%s_exact' % Type], out['d_%s' % Type] = r, exact, np.float64(d)
        if TYPES[Type] == 'cat':
            out['pairs.%s_terms' % Type] = terms

    for k, (Type, variables, depend_var, reverse) in enumerate(DEPENDENT):
        ref = SD.associations_dependent(df, Type, variables, depend_var, reverse=reverse, plot=False)
        assert list(ref.index) == variables
        r = ref.to_numpy(dtype='float64')
        assert np.isfinite(r).all() and (r >= 0).all() and (r <= 1).all(), (Type, r)
        res = [association_exact(df, depend_var, v, Type) if reverse else association_exact(df, v, depend_var, Type) for v in variables]
        exact = np.array([e for e, _ in res])
        assert float(np.abs(r - exact).max()) <= float(out['d_%s' % Type]) + 1e-15, (Type, depend_var)
        out['dependent.%d' % k], out['dependent.%d_exact' % k] = r, exact
        if TYPES[Type] == 'cat':
            out['dependent.%d_terms' % k] = np.array([t if t is not None else (np.nan,) * 4 for _, t in res])

    for k, (name, args) in enumerate(DIRECT):
        for a in args[:2]:
            assert not df[a].isnull().any()
        r = float(getattr(SD, name)(df, *args))
        e = direct_exact(df, name, args)
        print('%-24s %-24s ref %.17g exact %.17g' % (name, args, r, e), flush=True)
        assert np.isfinite(r) and abs(r - e) <= 1e-9 * max(1.0, abs(e))
        out['direct.%d' % k], out['direct.%d_exact' % k] = np.float64(r), np.float64(e)
    assert df.equals(before)
    np.savez_compressed(OUT, **out)
    with np.load(OUT, allow_pickle=False) as z:
        assert len(z.files) == len(out)
    print('wrote', OUT, '%.1f KB' % (os.path.getsize(OUT) / 1024), len(out), 'arrays')


if __name__ == '__main__':
    main()
