"""Numpy restatement of the modelled-data statistics (bayhunter_amd/datafits.py): per column of Y over rows
with integer weights, as numpy computes them on np.repeat(Y, w, axis=0).  Test code only."""
import numpy as np


def included(Y, err=None):
    """rows with no NaN among the columns and no non-zero err flag"""
    ok = ~np.isnan(Y).any(axis=1)
    if err is not None:
        ok &= ~(np.asarray(err) != 0).any(axis=1)
    return ok


def order_stats(Y, w, ranks):
    """values of 0-based ranks of every column of the expanded matrix: argsort + cumulative weights"""
    Y = np.asarray(Y, dtype=np.float64)
    w = np.asarray(w, dtype=np.int64)
    out = np.empty((len(ranks), Y.shape[1]))
    for c in range(Y.shape[1]):
        o = np.argsort(Y[:, c], kind='stable')
        cum = np.cumsum(w[o])
        idx = np.searchsorted(cum, np.asarray(ranks, dtype=np.int64), side='right')
        out[:, c] = Y[o[idx], c]
    return out


def lerp(a, b, t):
    d = b - a
    return np.where(t >= 0.5, b - d * (1 - t), a + d * t)


def percentiles(Y, w, q):
    W = int(np.sum(w))
    virt = np.true_divide(np.asarray(q, dtype=np.float64), 100) * (W - 1)
    lo = np.floor(virt).astype(np.int64)
    hi = np.ceil(virt).astype(np.int64)
    a, b = order_stats(Y, w, lo), order_stats(Y, w, hi)
    return lerp(a, b, (virt - lo)[:, None]), a, b


def bin_index(values, edges):
    i = np.searchsorted(edges, values, side='right') - 1
    i[values == edges[-1]] = edges.size - 2
    i[(i < 0) | (i > edges.size - 2)] = -1
    return i


def histogram(col, w, edges):
    b = bin_index(col, edges)
    keep = b >= 0
    return np.bincount(b[keep], weights=np.asarray(w)[keep], minlength=edges.size - 1).astype(np.int64)


def summarize(Y, w=None, q=(2.5, 16, 50, 84, 97.5), segs=None, nbins=100, err=None):
    """-> dict(mean, std, min, max, median, lower/upper order statistics, quantiles, hist per column, edges per
    segment, nmodels, nexcluded) of the included rows of Y [R, S]; segs: column ranges sharing edges"""
    Y = np.asarray(Y, dtype=np.float64)
    w = np.ones(Y.shape[0], dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    ok = included(Y, err)
    nex = int(w[~ok].sum())
    Y, w = Y[ok & (w > 0)], w[ok & (w > 0)]
    W = int(w.sum())
    wf = w.astype(np.float64)[:, None]
    mean = (wf * Y).sum(axis=0) / W
    std = np.sqrt((wf * (Y - mean) ** 2).sum(axis=0) / W)
    quant, lo, hi = percentiles(Y, w, q)
    m = order_stats(Y, w, [(W - 1) // 2, W // 2])
    segs = segs or [(0, Y.shape[1])]
    hist, edges = np.zeros((Y.shape[1], nbins), dtype=np.int64), []
    for a, b in segs:
        tmin, tmax = Y[:, a:b].min(), Y[:, a:b].max()
        if tmin == tmax:
            tmin, tmax = tmin - 0.5, tmax + 0.5
        e = np.linspace(tmin, tmax, nbins + 1)
        edges.append(e)
        for c in range(a, b):
            hist[c] = histogram(Y[:, c], w, e)
    return dict(mean=mean, std=std, min=Y.min(axis=0), max=Y.max(axis=0), median=(m[0] + m[1]) / 2.,
                lower=lo, upper=hi, quantiles=quant, hist=hist, edges=edges, nmodels=W, nexcluded=nex)
