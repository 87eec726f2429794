"""Plain numpy restatement of the scalar-parameter posterior (bayhunter_amd/scalars.py, csrc/pairs.hip): rows are
expanded with np.repeat, and np.median, np.histogram and np.histogram2d do the rest on the columns in the dtype in which
ChainPool.save() writes them -- what PlotFromStorage.plot_posterior_likes / _misfits / _vpvs / _noise / _nlayers
(src/Plotting.py:552-710) computes, without the figures.  Nothing here is shared with the code under test."""
import numpy as np

DTYPE = {'f4': np.float32, 'f8': np.float64, 'n': np.float64, 'pair': np.float64}


def hist2d_sets(D, weights, set_start, pairs, edges):
    """What bh_hist2d_sets counts: per set s (rows set_start[s]:set_start[s + 1]) and pair (cx, cy)
    np.histogram2d(x, y, bins=(edges[s][cx], edges[s][cy])) of the expanded columns, rows with a NaN in either left out
    -> int64 [sets, pairs, nb, nb].  (A set whose expansion would not fit in memory -- the eight weights of 2^30 -- goes
    through np.histogram2d's own `weights`: float64 sums of integers, exact below 2^53.)"""
    D = np.asarray(D, dtype=np.float64)
    S, nb = len(set_start) - 1, edges.shape[2] - 1
    w = np.ones(D.shape[0], dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    out = np.zeros((S, len(pairs), nb, nb), dtype=np.int64)
    for s in range(S):
        a, b = int(set_start[s]), int(set_start[s + 1])
        expand = w[a:b].sum() <= 10 ** 7
        assert w[a:b].sum() < 2 ** 53
        for i, (cx, cy) in enumerate(pairs):
            if expand:
                x, y, ws = np.repeat(D[a:b, cx], w[a:b]), np.repeat(D[a:b, cy], w[a:b]), None
            else:
                x, y, ws = D[a:b, cx], D[a:b, cy], w[a:b].astype(np.float64)
            ok = ~np.isnan(x) & ~np.isnan(y)
            h = np.histogram2d(x[ok], y[ok], bins=(edges[s, cx], edges[s, cy]), weights=None if ws is None else ws[ok])[0]
            assert np.array_equal(h, np.rint(h))
            out[s, i] = h.astype(np.int64)
    return out


def column(v, tag, nbins):
    """The per-column record of an expanded column `v` in its own dtype."""
    assert v.dtype == DTYPE[tag]
    const = bool(v.min() == v.max())
    if tag == 'n':
        bins = np.arange(np.min(v), np.max(v) + 2) - 0.5            # Plotting.py:615
    elif const:
        m = v.min()
        bins = [m - 1, m - 0.1, m + 0.1, m + 1]                     # Plotting.py:652-655, around the value itself
    else:
        bins = nbins
    counts, edges = np.histogram(v, bins=bins)
    cbins = (edges[:-1] + edges[1:]) / 2.                           # Plotting.py:558-559
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), constant=const,
                mean=float(np.mean(v.astype(np.float64))), std=float(np.std(v.astype(np.float64))),
                mode=float(cbins[np.argmax(counts)]), hist=(counts, edges))


def summarize(data, tags, names, weights=None, nbins=20, pairs=(), pair_bins=50):
    """The record scalars.summarize returns for the float64 matrix `data` [rows, K], or None without an included row of
    positive weight.  Rows with a NaN in a column that has statistics enter none of them (nexcluded)."""
    data = np.asarray(data, dtype=np.float64)
    K = data.shape[1]
    w = np.ones(data.shape[0], dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    nstat = sum(t != 'pair' for t in tags)
    inc = ~np.isnan(data[:, :nstat]).any(axis=1)
    if w[inc].sum() == 0:
        return None
    res = dict(nmodels=int(w[inc].sum()), nexcluded=int(w[~inc].sum()), pairs={})
    full = np.repeat(data[inc], w[inc], axis=0)
    for c in range(nstat):
        res[names[c]] = column(full[:, c].astype(DTYPE[tags[c]]), tags[c], nbins)
    finite = {}
    for c in range(K):
        if c < nstat:
            finite[c] = full[:, c]
        else:
            v = np.repeat(data[:, c], w)
            finite[c] = v[~np.isnan(v)]
            res['nmodels_' + names[c]] = int(finite[c].size)
            res['nexcluded_' + names[c]] = int(v.size - finite[c].size)
    allx = np.repeat(data, w, axis=0)
    for cx, cy in pairs:
        cx, cy = (names.index(c) if isinstance(c, str) else c for c in (cx, cy))
        if finite[cx].size == 0 or finite[cy].size == 0:
            nan = np.full(pair_bins + 1, np.nan)
            rec = dict(counts=np.zeros((pair_bins, pair_bins), dtype=np.int64), xedges=nan, yedges=nan, mode=(np.nan, np.nan))
        else:
            xe = np.histogram(finite[cx], bins=pair_bins)[1]
            ye = np.histogram(finite[cy], bins=pair_bins)[1]
            ok = ~np.isnan(allx[:, cx]) & ~np.isnan(allx[:, cy])
            h = np.histogram2d(allx[ok, cx], allx[ok, cy], bins=(xe, ye))[0].astype(np.int64)
            xi, yi = np.unravel_index(h.argmax(), h.shape)
            rec = dict(counts=h, xedges=xe, yedges=ye, mode=((xe[xi] + xe[xi + 1]) / 2., (ye[yi] + ye[yi + 1]) / 2.))
        res['pairs'][(names[cx], names[cy])] = rec
    return res


def same(a, b):
    """Equal bit for bit, NaN equal to NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


EXACT = ('median', 'min', 'max', 'mode', 'constant')


def assert_record(got, want, names, nstat, mean_std=None):
    """`got` (scalars.summarize's dict) against `want` (summarize above): everything but mean / std bit for bit;
    mean_std(got column, want column, name) checks those two."""
    assert got['nmodels'] == want['nmodels'] and got['nexcluded'] == want['nexcluded']
    for name in names[:nstat]:
        g, w = got[name], want[name]
        for k in EXACT:
            assert same(g[k], w[k]), (name, k, g[k], w[k])
        assert np.array_equal(g['hist'][0], w['hist'][0]), (name, g['hist'][0], w['hist'][0])
        assert g['hist'][1].dtype == w['hist'][1].dtype and same(g['hist'][1], w['hist'][1]), name
        if mean_std is not None:
            mean_std(g, w, name)
    for name in names[nstat:]:
        for k in ('nmodels_' + name, 'nexcluded_' + name):
            assert got[k] == want[k], k
    assert list(got['pairs']) == list(want['pairs'])
    for p, w in want['pairs'].items():
        g = got['pairs'][p]
        assert np.array_equal(g['counts'], w['counts']), p
        assert same(g['xedges'], w['xedges']) and same(g['yedges'], w['yedges']) and same(g['mode'], w['mode']), p
