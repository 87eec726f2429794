"""Plain numpy restatement of the depth-to-depth second moment (bayhunter_amd/covariance.py, csrc/depthcov.hip): a row's
Vs on the depth grid is posterior_ref.interp, the centred values are one float64 subtraction as in the library, and every
sum over the weighted rows is taken in np.longdouble.  Also the cases both tiers run.  Test code only."""
import numpy as np

import posterior_ref as pref

LD = np.longdouble
WIDTH = 12                       # six nuclei at most


def columns(rows, dep, extra=None):
    """-> (X [R, K] float64: Vs on dep, then the extra columns; has a model [R])."""
    X, n, _ = pref.interp(rows, dep)
    if extra is not None and extra.shape[1]:
        X = np.hstack((X, np.asarray(extra, dtype=np.float64)))
    return X, n >= 1


def moments(rows, weights, extra, set_start, dep, center):
    """What bh_depthcov_sets returns, and what bounds its error: per set over the rows with w > 0 and a model, with
    d = fl(x - center) in float64 and everything after it in long double,

        S = sum w d d^T, r1 = sum w d, total = sum w, absS = sum w |d| |d|^T, absr1 = sum w |d|, terms = such rows

    -> dict of arrays with one entry per set (S, absS [sets, K, K] and r1, absr1 [sets, K] long double)."""
    X, has = columns(rows, dep, extra)
    R, K = X.shape
    w = np.ones(R, dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    Z = len(set_start) - 1
    out = dict(S=np.zeros((Z, K, K), dtype=LD), absS=np.zeros((Z, K, K), dtype=LD), r1=np.zeros((Z, K), dtype=LD),
               absr1=np.zeros((Z, K), dtype=LD), total=np.zeros(Z, dtype=np.int64), terms=np.zeros(Z, dtype=np.int64))
    for z in range(Z):
        a, b = int(set_start[z]), int(set_start[z + 1])
        keep = np.nonzero((w[a:b] > 0) & has[a:b])[0] + a
        if keep.size == 0:
            continue
        d = (X[keep] - np.asarray(center[z], dtype=np.float64)[None, :]).astype(LD)
        wl = w[keep].astype(LD)[:, None]
        out['S'][z] = (wl * d).T @ d
        out['absS'][z] = (wl * np.abs(d)).T @ np.abs(d)
        out['r1'][z] = (wl * d).sum(axis=0)
        out['absr1'][z] = (wl * np.abs(d)).sum(axis=0)
        out['total'][z] = w[keep].sum()
        out['terms'][z] = keep.size
    return out


def cov_corr(S, r1, W):
    """(S - r1 r1^T / W) / W and its correlation in long double; NaN where a variance is not above 0."""
    S, r1, W = np.asarray(S, dtype=LD), np.asarray(r1, dtype=LD), LD(W)
    cov = (S - np.outer(r1, r1) / W) / W
    var = np.diagonal(cov)
    with np.errstate(invalid='ignore', divide='ignore'):
        std = np.sqrt(np.where(var > 0, var, np.nan))
        corr = cov / np.outer(std, std)
    return cov, corr


def weighted_means(rows, weights, extra, set_start, dep):
    """A centre per set as the package makes it: the float64 weighted mean of the counted rows (zeros for a set without)."""
    X, has = columns(rows, dep, extra)
    w = np.ones(X.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    Z = len(set_start) - 1
    c = np.zeros((Z, X.shape[1]))
    for z in range(Z):
        a, b = int(set_start[z]), int(set_start[z + 1])
        keep = (w[a:b] > 0) & has[a:b]
        if keep.any():
            c[z] = (w[a:b][keep, None] * X[a:b][keep]).sum(axis=0) / w[a:b][keep].sum()
    return c


# ---- the cases of both tiers ---------------------------------------------------------------------------------------

def random_rows(rng, R, dtype, min_nuclei=1):
    """R rows [vs(n) | z(n) | NaN ..] of WIDTH columns with n = min_nuclei .. 6 nuclei, in `dtype`."""
    rows = np.full((R, WIDTH), np.nan)
    n = rng.integers(min_nuclei, WIDTH // 2 + 1, size=R)
    for r in range(R):
        rows[r, :n[r]] = rng.uniform(2., 5., n[r])
        rows[r, n[r]:2 * n[r]] = np.sort(rng.uniform(0., 60., n[r]))
    return rows.astype(dtype)


def case(B, ndep, nextra, fp64, weighted, seed=0):
    """The shapes of the issue: sets of 1, 3, 4, B, B + 1 and 2 B + 5 rows, an empty set between them, and a set of 5
    rows whose weights are all 0 (unweighted: whose rows are all NaN); one all-NaN row and one one-nucleus row inside
    the set of B + 1; weights in [0, 40] with about 10 % zeros and one of 2^31 - 1; dep with a point exactly on the first
    interface of the first row of the set of B rows and a point below every model.
    -> dict(rows, weights (int32 or None), extra ([R, nextra] or None), set_start, dep, center, counts)."""
    rng = np.random.default_rng(1000 * ndep + 10 * nextra + 2 * int(fp64) + int(weighted) + 7919 * seed)
    counts = [1, 3, 0, 4, B, 5, B + 1, 2 * B + 5]
    set_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    R = int(set_start[-1])
    dtype = np.float64 if fp64 else np.float32
    rows = random_rows(rng, R, dtype)
    first = int(set_start[4])
    rows[first] = random_rows(rng, 1, dtype, min_nuclei=3)[0]
    at = int(set_start[6])
    rows[at + 2] = np.nan                                              # an all-NaN row
    rows[at + 5] = np.nan
    rows[at + 5, :2] = np.asarray([3.25, 11.], dtype=dtype)           # a one-nucleus row: a half-space
    weights = None
    if weighted:
        weights = rng.integers(0, 41, size=R).astype(np.int64)
        weights[rng.uniform(size=R) < 0.1] = 0
        weights[first + 1] = 2 ** 31 - 1
        weights[first] = 17
        weights[set_start[[0, 1, 3]]] = (5, 1, 40)                    # (the small sets keep a row that counts)
        weights[set_start[5]:set_start[6]] = 0                        # a set whose rows all have weight 0
        weights = weights.astype(np.int32)
    else:
        rows[set_start[5]:set_start[6]] = np.nan                      # (without weights: a set of rows without a model)
    n = int((~np.isnan(rows[first])).sum() // 2)
    z = rows[first, n:2 * n].astype(np.float64)
    iface = (z[0] + z[1]) / 2. - 0.                                    # the walk's own arithmetic for the first interface
    dep = np.unique(np.concatenate((np.linspace(0., 70., max(ndep - 2, 0)), [iface, 200.])))
    assert dep.size == ndep and iface in dep
    extra = None
    if nextra:
        extra = np.ascontiguousarray(rng.uniform(1.6, 1.9, size=(R, nextra)) * (1. + np.arange(nextra))[None, :])
    center = weighted_means(rows, weights, extra, set_start, dep)
    return dict(rows=rows, weights=weights, extra=extra, set_start=set_start, dep=dep, center=center, counts=counts)
