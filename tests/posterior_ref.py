"""Vectorised numpy restatement of the reference's posterior statistics, written from the cited lines:

    Model.get_stepmodel / get_interpmodel       src/Models.py:55-70, 94-113
    ModelMatrix._delete_nanmodels               src/Models.py:116-126
    ModelMatrix.get_singlemodels                src/Models.py:160-226
    PlotFromStorage._plot_bestmodels_hist       src/Plotting.py:462-536 (density + interface histogram)
    PlotFromStorage.plot_posterior_nlayers      src/Plotting.py:607-625
    PlotFromStorage.get_outliers                src/Plotting.py:113-154

Rows carry integer weights; statistics are those of the matrix with every row repeated `weight` times.
Test code only."""
import glob
import os

import numpy as np

VS_INTERVAL = 0.025


def split_rows(rows):
    """-> (n nuclei [R], vs [R, maxn], interface depths [R, maxn - 1] (NaN past n - 1)) in fp64"""
    rows = np.asarray(rows, dtype=np.float64)
    R, W = rows.shape
    nan = np.isnan(rows)
    c = np.where(nan.any(axis=1), nan.argmax(axis=1), W)
    n = c // 2
    maxn = W // 2
    k = np.arange(maxn)[None, :]
    have = k < n[:, None]
    ridx = np.arange(R)[:, None]
    vs = np.where(have, rows[ridx, np.minimum(k, W - 1)], np.nan)
    z = np.where(have, rows[ridx, np.minimum(c[:, None] - n[:, None] + k, W - 1)], np.nan)
    z_disc = (z[:, :-1] + z[:, 1:]) / 2.
    h = z_disc - np.concatenate((np.zeros((R, 1)), z_disc[:, :-1]), axis=1)
    return n, vs, np.cumsum(h, axis=1)


def interp(rows, dep, chunk=4096):
    """Vs of every row at every depth [R, D]: the layer of depth x is the number of interfaces <= x
    (np.interp over the step knots: a point on an interface takes the deeper layer)"""
    n, vs, D = split_rows(rows)
    dep = np.asarray(dep, dtype=np.float64)
    out = np.empty((vs.shape[0], dep.size))
    for lo in range(0, vs.shape[0], chunk):
        hi = lo + chunk
        layer = (D[lo:hi, None, :] <= dep[None, :, None]).sum(axis=2)
        out[lo:hi] = np.take_along_axis(vs[lo:hi], layer, axis=1)
    return out, n, D


def bin_index(values, edges):
    i = np.searchsorted(edges, values, side='right') - 1
    i[values == edges[-1]] = edges.size - 2
    i[(i < 0) | (i > edges.size - 2)] = -1
    return i


def vs_round(vs):
    vs_floor = np.floor(vs)
    return np.round((vs - vs_floor) * 40) / 40 + vs_floor


def hist_grids(dep_int):
    if dep_int is None:
        return np.linspace(0, 100, 201), np.linspace(0, 100, 101)
    maxdepth = int(np.ceil(dep_int.max()))
    interp_ = dep_int[1] - dep_int[0]
    return (np.arange(dep_int[0], dep_int[-1] + interp_ / 2., interp_ / 2.),
            np.arange(0, maxdepth + 2 * interp_, interp_))


def stepmodel(row):
    m = np.asarray(row, dtype=np.float64)
    m = m[~np.isnan(m)]
    n = m.size // 2
    vs, z = m[:n], m[-n:]
    zd = (z[:-1] + z[1:]) / 2.
    dep = np.cumsum(np.concatenate((zd - np.concatenate(([0.], zd[:-1])), [0.])))
    dep_step = np.concatenate(([0.], np.repeat(dep, 2)[:-1]))
    dep_step[-1] = max(150., dep_step[-1] * 2.5)
    return np.repeat(vs, 2), dep_step


def summarize(rows, weights=None, dep_int=None, misfits=None):
    """The package's summarize() result, computed on the expanded matrix with numpy"""
    rows = np.asarray(rows)
    w = np.ones(rows.shape[0], dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    valid = ~np.isnan(rows.astype(np.float64)).all(axis=1)
    hist_dep = dep_int
    dep_int = np.linspace(0, 100, 201) if dep_int is None else np.asarray(dep_int, dtype=np.float64)
    keep = valid & (w > 0)
    vsi, n, _ = interp(rows[keep], dep_int)
    vss = np.repeat(vsi, w[keep], axis=0)
    mean, median, std = vss.mean(axis=0), np.median(vss, axis=0), vss.std(axis=0)
    vmin, vmax = vss.min(), vss.max()
    vedges = np.linspace(vmin, vmax, int((vmax - vmin) / VS_INTERVAL) + 1)
    vb = bin_index(vss.ravel(), vedges).reshape(vss.shape)
    db = np.broadcast_to(bin_index(dep_int, dep_int), vss.shape)
    mh = np.zeros((dep_int.size - 1, vedges.size - 1), dtype=np.int64)
    np.add.at(mh, (db.ravel(), vb.ravel()), 1)
    single = dict(mean=(mean, dep_int), median=(median, dep_int),
                  minmax=(np.array((vss.min(axis=0), vss.max(axis=0))), dep_int),
                  stdminmax=(np.array((mean - std, mean + std)), dep_int),
                  mode=(((vedges[:-1] + vedges[1:]) / 2.)[np.argmax(mh, axis=1)], (dep_int[:-1] + dep_int[1:]) / 2.))
    if misfits is not None:
        mis = np.repeat(np.asarray(misfits, dtype=np.float64), w)
        single['minmisfit'] = stepmodel(np.repeat(rows, w, axis=0)[np.argmin(mis)])
    dep2, depbins = hist_grids(None if hist_dep is None else np.asarray(hist_dep, dtype=np.float64))
    v2 = np.repeat(interp(rows[keep], dep2)[0], w[keep], axis=0)
    vsb = np.arange(vs_round(v2.min()) - 2 * VS_INTERVAL, vs_round(v2.max()) + 3 * VS_INTERVAL, VS_INTERVAL)
    b1 = bin_index(v2.ravel(), vsb)
    b2 = np.broadcast_to(bin_index(dep2, depbins), v2.shape).ravel()
    ok = (b1 >= 0) & (b2 >= 0)
    h2 = np.zeros((vsb.size - 1, depbins.size - 1), dtype=np.int64)
    np.add.at(h2, (b1[ok], b2[ok]), 1)
    _, _, D = split_rows(rows[keep])
    ifd = np.repeat(D, w[keep], axis=0).ravel()
    ifd = ifd[~np.isnan(ifd)]
    nl = np.bincount(n, weights=w[keep], minlength=rows.shape[1] // 2 + 1).astype(np.int64)
    return dict(singlemodels=single, hist2d=(h2, vsb, depbins),
                interfaces=(np.histogram(ifd, depbins)[0], depbins), nlayers=nl, nmodels=int(w[keep].sum()))


def weighted_median(vals, w):
    """np.median over the columns of np.repeat(vals, w, 0), without the repetition"""
    order = np.argsort(vals, axis=0, kind='stable')
    sv = np.take_along_axis(vals, order, axis=0)
    cw = np.cumsum(w[order], axis=0)
    W = int(w.sum())
    pick = lambda r: np.take_along_axis(sv, (cw <= r).sum(axis=0)[None, :], axis=0)[0]
    return (pick((W - 1) // 2) + pick(W // 2)) / 2.


def outliers_from_files(datapath, dev=0.05):
    """get_outliers over the c*_p2likes.npy files of a directory -> chain indices"""
    files = sorted(glob.glob(os.path.join(datapath, 'c*_p2likes.npy')))
    idx = np.array([int(os.path.basename(f).split('_')[0][1:]) for f in files])
    med = np.array([np.median(np.load(f)) for f in files], dtype=np.float64)
    maxlike = med.max()
    scores = med / maxlike if maxlike > 0 else maxlike / med
    return idx[(1 - scores) > dev]
