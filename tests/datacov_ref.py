"""Plain numpy restatement of the cross moment of Vs(z) and the modelled data (bayhunter_amd/datacov.py,
csrc/datacov.hip): the model columns are depthcov_ref.columns, the centred values are one float64 subtraction as in the
library, and every sum over the weighted rows is taken in np.longdouble.  Also the cases both tiers run.  Test code only."""
import numpy as np

import depthcov_ref as dref

LD = np.longdouble
NFLAGS = 2


def counts(rows, weights, Y, err, dep):
    """-> (w [R] int64, the rows that count [R] bool): weight above 0, a model, every flag 0, no NaN among the data."""
    _, has = dref.columns(rows, dep)
    R = rows.shape[0]
    w = np.ones(R, dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    ok = (w > 0) & has & ~np.isnan(Y).any(axis=1)
    if err is not None and err.shape[1]:
        ok &= ~(np.asarray(err) != 0).any(axis=1)
    return w, ok


def moments(rows, weights, extra, Y, err, set_start, dep, cx, cy):
    """What bh_datacov_sets returns, and what bounds its error: per set over the rows that count, with dx = fl(x - cx)
    and dy = fl(y - cy) in float64 and everything after them in long double,

        C = sum w dx dy^T, r1x = sum w dx, r1y = sum w dy, qx = sum w dx^2, qy = sum w dy^2, total = sum w,
        excluded = sum of w over the rows with w > 0 that do not count,
        absC = sum w |dx| |dy|^T, absr1x = sum w |dx|, absr1y = sum w |dy|, terms = rows that count

    -> dict of arrays with one entry per set (long double but total, excluded, terms)."""
    X, _ = dref.columns(rows, dep, extra)
    Y = np.asarray(Y, dtype=np.float64)
    w, ok = counts(rows, weights, Y, err, dep)
    K, S, Z = X.shape[1], Y.shape[1], len(set_start) - 1
    z2 = lambda *s: np.zeros(s, dtype=LD)
    out = dict(C=z2(Z, K, S), absC=z2(Z, K, S), r1x=z2(Z, K), absr1x=z2(Z, K), r1y=z2(Z, S), absr1y=z2(Z, S), qx=z2(Z, K),
               qy=z2(Z, S), total=np.zeros(Z, dtype=np.int64), excluded=np.zeros(Z, dtype=np.int64),
               terms=np.zeros(Z, dtype=np.int64))
    for z in range(Z):
        a, b = int(set_start[z]), int(set_start[z + 1])
        keep = np.nonzero(ok[a:b])[0] + a
        out['excluded'][z] = w[a:b][(w[a:b] > 0) & ~ok[a:b]].sum()
        if keep.size == 0:
            continue
        dx = (X[keep] - np.asarray(cx[z], dtype=np.float64)[None, :]).astype(LD)
        dy = (Y[keep] - np.asarray(cy[z], dtype=np.float64)[None, :]).astype(LD)
        wl = w[keep].astype(LD)[:, None]
        out['C'][z] = (wl * dx).T @ dy
        out['absC'][z] = (wl * np.abs(dx)).T @ np.abs(dy)
        out['r1x'][z], out['r1y'][z] = (wl * dx).sum(axis=0), (wl * dy).sum(axis=0)
        out['absr1x'][z], out['absr1y'][z] = (wl * np.abs(dx)).sum(axis=0), (wl * np.abs(dy)).sum(axis=0)
        out['qx'][z], out['qy'][z] = (wl * dx * dx).sum(axis=0), (wl * dy * dy).sum(axis=0)
        out['total'][z] = w[keep].sum()
        out['terms'][z] = keep.size
    return out


def cov(m, z):
    """(C - r1x r1y^T / W) / W of set z of moments' dict, in long double."""
    W = LD(m['total'][z])
    return (m['C'][z] - np.outer(m['r1x'][z], m['r1y'][z]) / W) / W


def variances(m, z):
    """((qx - r1x^2 / W) / W, (qy - r1y^2 / W) / W) of set z, in long double."""
    W = LD(m['total'][z])
    return (m['qx'][z] - m['r1x'][z] ** 2 / W) / W, (m['qy'][z] - m['r1y'][z] ** 2 / W) / W


def weighted_means(rows, weights, extra, Y, err, set_start, dep):
    """The centres (cx [sets, K], cy [sets, S]) as the package makes them: float64 weighted means of the rows that
    count (zeros for a set without)."""
    X, _ = dref.columns(rows, dep, extra)
    w, ok = counts(rows, weights, Y, err, dep)
    Z = len(set_start) - 1
    cx, cy = np.zeros((Z, X.shape[1])), np.zeros((Z, Y.shape[1]))
    for z in range(Z):
        a, b = int(set_start[z]), int(set_start[z + 1])
        k = ok[a:b]
        if k.any():
            wz = w[a:b][k].astype(np.float64)
            cx[z] = (wz[:, None] * X[a:b][k]).sum(axis=0) / wz.sum()
            cy[z] = (wz[:, None] * Y[a:b][k]).sum(axis=0) / wz.sum()
    return cx, cy


def case(B, ndep, nextra, S, fp64, weighted, nans=True, seed=0):
    """depthcov_ref.case's rows, weights, extra, sets and grid (sets of 1, 3, 0, 4, B, 5, B + 1 and 2 B + 5 rows; set 2
    empty, set 5 without a row that counts) with synthetic data beside them: Y [R, S] -- a part that follows the row's
    first velocity, so that the moments are not all noise -- and err [R, NFLAGS] with about 4 % of the rows flagged;
    with `nans` about 4 % of the rows hold a single NaN in column S - 1 (a column of the last group of data columns).
    The first row of every set of 1, 3 and 4 rows counts.
    -> depthcov_ref.case's dict with Y, err, cx, cy (the means over the rows that count) and S."""
    c = dref.case(B, ndep, nextra, fp64, weighted, seed)
    rng = np.random.default_rng(31 * S + 1000 * ndep + 10 * nextra + 2 * int(fp64) + int(weighted) + 7919 * seed)
    R = c['rows'].shape[0]
    v0 = np.nan_to_num(c['rows'][:, 0].astype(np.float64), nan=3.)
    Y = rng.uniform(-1., 4., size=(R, S)) + 0.5 * v0[:, None] * np.cos(np.arange(S))[None, :]
    err = np.zeros((R, NFLAGS), dtype=np.int32)
    flagged = rng.uniform(size=R) < 0.04
    err[flagged, rng.integers(0, NFLAGS, size=int(flagged.sum()))] = rng.integers(1, 4, size=int(flagged.sum()))
    holes = (rng.uniform(size=R) < 0.04) if nans else np.zeros(R, dtype=bool)
    keep = c['set_start'][[0, 1, 3]]
    err[keep] = 0
    holes[keep] = False
    Y[holes, S - 1] = np.nan
    if nans:
        assert holes[c['set_start'][7]:].any() and flagged.any()
    c.update(Y=Y, err=err, S=S)
    c['cx'], c['cy'] = weighted_means(c['rows'], c['weights'], c['extra'], Y, err, c['set_start'], c['dep'])
    del c['center']
    return c
