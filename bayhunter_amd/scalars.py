"""Posterior of the sampler's scalar parameters, on the device: likelihood, misfits, Vp/Vs, noise and layer count.

What the reference shows in PlotFromStorage.plot_posterior_likes / _misfits / _vpvs / _noise / _nlayers / _others
(src/Plotting.py:552-710): per parameter the median, a histogram and its mode.  Here also min / max / mean / std, and
the joint histograms of chosen pairs of parameters (Moho depth against Vp/Vs, the sigma of one target against
another's, layer count against likelihood), for one set of rows or for every station of a network in one pass.

Every row carries an integer weight; the result equals the reference's on the columns in which each row is repeated
`weight` times.  The per-column part is the weighted column reduction of datafits (bh_datafits_* / bh_datafits_sets_*
on a small matrix), the pairs are bh_hist2d_sets (csrc/pairs.hip).  Edges are made here with numpy, in the dtype in
which ChainPool.save() writes the column, as np.histogram makes them there.

Where this leaves the reference on purpose: a column is `constant` when min == max.  The reference tests
np.std(data) == 0, which depends on the rounding of a pairwise sum and can come out non-zero for a column of identical
values; and it centres the constant's edges on np.mean(data), here on the value itself.
"""
import numpy as np

from . import _device, _lib, datafits as df, selection as sel      # (`selection` is a parameter of the entry points)
from .moho import outer_edges

F4, F8, COUNT, PAIR = 'f4', 'f8', 'n', 'pair'      # the tag of a column (Columns)


def NAMES(ntargets, refs, moho=False):
    """The columns in their fixed order:
    like | misfit:<ref> per target | misfit:joint | vpvs | corr:<ref>, sigma:<ref> per target | nlayers | (moho)"""
    refs = [str(r) for r in refs]
    if len(refs) != int(ntargets):
        raise ValueError("one ref per target")
    names = ['like'] + ['misfit:%s' % r for r in refs] + ['misfit:joint', 'vpvs']
    for r in refs:
        names += ['corr:%s' % r, 'sigma:%s' % r]
    return names + ['nlayers'] + (['moho'] if moho else [])


def TAGS(ntargets, moho=False):
    """The tag of every column of NAMES: the dtype save() writes it in -- like and vpvs float32, misfits and noise
    float32 widened to float64 (ChainPool.weighted), the layer count a float64 count, moho for pairs only."""
    return [F4] + [F8] * (ntargets + 1) + [F4] + [F8] * (2 * ntargets) + [COUNT] + ([PAIR] if moho else [])


class Columns(object):
    """A float64 matrix [rows, K] (numpy or a torch tensor) with a name and a tag per column:

    'f4'    the column is float32 in the reference (its values here are float32 values, widened): median, edges and
            mode are computed in float32
    'f8'    float64
    'n'     a count (float64): the histogram has one bin per integer, edges arange(min, max + 2) - 0.5
    'pair'  takes part in pairs only, not in the per-column statistics; may hold NaN.  These columns come last."""

    def __init__(self, data, tags, names=None):
        self.data = data
        self.tags = list(tags)
        K = len(self.tags)
        self.names = ['c%d' % c for c in range(K)] if names is None else [str(n) for n in names]
        if len(data.shape) != 2 or data.shape[1] != K or len(self.names) != K or len(set(self.names)) != K:
            raise ValueError("cols: a matrix [rows, K] with one tag and one distinct name per column")
        if any(t not in (F4, F8, COUNT, PAIR) for t in self.tags):
            raise ValueError("tags: 'f4', 'f8', 'n' or 'pair'")
        self.nstat = sum(t != PAIR for t in self.tags)
        if self.nstat < 1 or any(t == PAIR for t in self.tags[:self.nstat]):
            raise ValueError("cols: one column with statistics at least, the 'pair' columns last")

    def index(self, c):
        if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
            if not 0 <= c < len(self.names):
                raise ValueError("pairs: column %d of %d" % (c, len(self.names)))
            return int(c)
        if c not in self.names:
            raise ValueError("pairs: no column %r (there are %s)" % (c, ', '.join(self.names)))
        return self.names.index(c)


# ---- the rules, without a device ------------------------------------------------------------------------

def _dtype(tag):
    return np.float32 if tag == F4 else np.float64


def median_of(lo, hi, W, tag):
    """np.median of the expanded column from its two middle order statistics (ranks (W - 1) // 2 and W // 2), in the
    column's dtype: the middle value, or the mean of the two, for float32 rounded to float32 -> float64."""
    dt = _dtype(tag)
    lo, hi = dt(lo), dt(hi)
    return np.float64(lo if W % 2 else (lo + hi) / dt(2))


def column_edges(vmin, vmax, tag, nbins):
    """The histogram edges of a column with the given extremes, in the column's dtype: np.histogram's own for
    bins=nbins (np.linspace in that dtype); for a count arange(min, max + 2) - 0.5 (Plotting.py:615); for a constant
    column [m - 1, m - 0.1, m + 0.1, m + 1] (Plotting.py:652-655)."""
    dt = _dtype(tag)
    lo, hi = dt(vmin), dt(vmax)
    if tag == COUNT:
        return np.arange(lo, hi + 2) - 0.5
    if lo == hi:
        return np.asarray([lo - 1, lo - 0.1, lo + 0.1, lo + 1])
    return np.linspace(lo, hi, int(nbins) + 1, dtype=dt)


def mode_of(counts, edges):
    """The centre of the first fullest bin (Plotting.py:558-559), in the edges' dtype -> float64."""
    centres = (edges[:-1] + edges[1:]) / 2.
    return np.float64(centres[np.argmax(counts)])


def pair_mode(counts, xedges, yedges):
    """(x, y): the cell centres of the first maximum in C order."""
    xi, yi = np.unravel_index(counts.argmax(), counts.shape)
    return (xedges[xi] + xedges[xi + 1]) / 2., (yedges[yi] + yedges[yi + 1]) / 2.


def padded_edges(edges, nedges):
    """`edges` (ascending) as float64 filled up to `nedges` with ascending values above its last."""
    e = np.asarray(edges, dtype=np.float64)
    pad = e[-1] + (1. + abs(e[-1])) * np.arange(1, nedges - e.size + 1)
    return np.concatenate((e, pad))


def unpadded_hist(hist, nb):
    """The first nb bins of a histogram over padded_edges: a value on the last true edge lies in the first padding bin
    there and in the closed last bin here."""
    h = hist[:nb].copy()
    if hist.size > nb:
        h[-1] += hist[nb]
    return h


def _pair_list(cols, pairs, pair_bins):
    pairs = [(cols.index(x), cols.index(y)) for x, y in pairs]
    if len(pairs) > _lib.PAIRS_MAX:
        raise ValueError("pairs: at most %d" % _lib.PAIRS_MAX)
    if pairs and not 1 <= int(pair_bins) <= _lib.PAIRS_MAX_EDGES - 1:
        raise ValueError("pair_bins: 1 to %d" % (_lib.PAIRS_MAX_EDGES - 1))
    return pairs


# ---- one set or many, on the device -------------------------------------------------------------------------

def _summarize(cols, set_start, weights, nbins, pairs, pair_bins, device):
    import torch
    if not isinstance(cols, Columns):
        raise ValueError("cols: a scalars.Columns")
    if int(nbins) < 1:
        raise ValueError("nbins >= 1")
    pairs = _pair_list(cols, pairs, pair_bins)
    K, nstat, tags, names = len(cols.tags), cols.nstat, cols.tags, cols.names
    dev = _device.torch_device(device)
    M = _device.to_device(cols.data, torch.float64, dev)
    if not M.is_contiguous():
        M = M.contiguous()
    R = M.shape[0]
    w = None if weights is None else _device.to_device(weights, torch.int32, dev)
    if w is not None and w.numel() != R:
        raise ValueError("one weight per row")
    set_start, S = sel.check_set_start(set_start, R)
    if S > _lib.PAIRS_MAX_SETS:
        raise ValueError("at most %d sets" % _lib.PAIRS_MAX_SETS)
    results, failed = [None] * S, {}
    if R == 0:
        return sel.SetList(results, {z: "empty selection: no rows" for z in range(S)})
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    handle = lambda Y, n: df._FitsSets(Y, n, w, None, set_start, stream)     # summarize(): the one set [0, R]
    with torch.cuda.device(dev):
        with handle(M, nstat) as f:
            s = f.scan()
            live = s['status'] == 0
            W = np.where(live, s['total'], 0)
            ranks = np.stack(((W - 1) // 2, W // 2), axis=1) * live[:, None]
            own = [[column_edges(s['vmin'][z, c], s['vmax'][z, c], tags[c], nbins) for c in range(nstat)] if live[z]
                   else None for z in range(S)]
            NE = max([e.size for es in own if es is not None for e in es] + [2])
            edges = np.zeros((S, nstat, NE))
            edges[:] = np.arange(NE)                        # (a set left out: anything ascending)
            for z in range(S):
                if live[z]:
                    edges[z] = [padded_edges(e, NE) for e in own[z]]
                else:
                    failed[z] = f.status_text(s['status'][z])
            ost, hist, std = f.finish(ranks, edges, np.arange(nstat, dtype=np.int32))
        extra = {}
        for k in range(nstat, K):                           # a column of the pairs alone: its weight and extremes
            with handle(M[:, k:k + 1], 1) as f:
                extra[k] = f.scan()
        h2 = pe = None
        if pairs:
            pb = int(pair_bins)
            pe = np.zeros((S, K, pb + 1))
            pe[:] = np.arange(pb + 1)
            for c in sorted(set(c for p in pairs for c in p)):
                sc, cc = (s, c) if c < nstat else (extra[c], 0)
                for z in np.nonzero(sc['status'] == 0)[0]:
                    pe[z, c] = outer_edges(sc['vmin'][z, cc], sc['vmax'][z, cc], pb)
            pr = np.ascontiguousarray(pairs, dtype=np.int32)
            h2 = np.zeros((S, len(pairs), pb, pb), dtype=np.int64)
            _lib.check(lib.bh_hist2d_sets(M.data_ptr(), R, M.stride(0), K, None if w is None else w.data_ptr(),
                                          set_start.ctypes.data, S, pr.ctypes.data, len(pairs), pe.ctypes.data, pb + 1,
                                          h2.ctypes.data, stream))
    for z in np.nonzero(live)[0]:
        d = dict(nmodels=int(s['total'][z]), nexcluded=int(s['excluded'][z]), pairs={})
        for c in range(nstat):
            e = own[z][c]
            counts = unpadded_hist(hist[z, c], e.size - 1)
            d[names[c]] = dict(median=median_of(ost[z, 0, c], ost[z, 1, c], int(W[z]), tags[c]), mean=s['mean'][z, c],
                               std=std[z, c], min=s['vmin'][z, c], max=s['vmax'][z, c], mode=mode_of(counts, e),
                               constant=bool(s['vmin'][z, c] == s['vmax'][z, c]), hist=(counts, e))
        for k in range(nstat, K):
            d['nmodels_' + names[k]] = int(extra[k]['total'][z])
            d['nexcluded_' + names[k]] = int(extra[k]['excluded'][z])
        for i, (cx, cy) in enumerate(pairs):
            has = all((c < nstat) or extra[c]['status'][z] == 0 for c in (cx, cy))
            xe = pe[z, cx].copy() if has else np.full(pe.shape[2], np.nan)
            ye = pe[z, cy].copy() if has else np.full(pe.shape[2], np.nan)
            d['pairs'][(names[cx], names[cy])] = dict(counts=h2[z, i], xedges=xe, yedges=ye,
                                                      mode=pair_mode(h2[z, i], xe, ye))
        results[z] = d
    return sel.SetList(results, failed)


def summarize(cols, weights=None, nbins=20, pairs=(), pair_bins=50, device=None):
    """Statistics of the columns `cols` (a Columns) over rows with integer `weights` (>= 0, default 1 each).

    pairs       pairs of columns (names or indices) for joint histograms of pair_bins x pair_bins cells (<= 64)

    -> dict(nmodels (the weight total), nexcluded (weighted rows with a NaN in a column that has statistics: they enter
            none of them), <column name> = dict(median, min, max (exact; median: np.median of the expanded column in
            the column's dtype), mean, std (float64, from the reduction), constant (min == max; module docstring),
            hist = (counts, edges) (what np.histogram returns for the expanded column in its dtype: bins=nbins, the
            count's or the constant's edges), mode (the centre of the first fullest bin)) for every column but the
            'pair' ones, nmodels_<name>, nexcluded_<name> for a 'pair' column (weighted rows with / without a value),
            pairs = {(x name, y name): dict(counts [pair_bins, pair_bins] (x first, as np.histogram2d), xedges, yedges
            (float64 outer_edges of the column's extremes over the rows that count in it), mode = (x, y))}; a pair
            with a column that has no value at all: zero counts, NaN edges and mode).
    ValueError for an empty selection."""
    rows = cols.data.shape[0] if isinstance(cols, Columns) else 0
    res = _summarize(cols, [0, rows], weights, nbins, pairs, pair_bins, device)
    if res[0] is None:
        raise ValueError(res.failed[0])
    return res[0]


def summarize_sets(cols, set_start, weights=None, nbins=20, pairs=(), pair_bins=50, device=None):
    """summarize() of every set of rows in one pass: set s is rows set_start[s]:set_start[s + 1] (set_start [sets + 1],
    ascending from 0 to the number of rows; a set may be empty).  One segmented reduction (bh_datafits_sets_*) and one
    bh_hist2d_sets launch for all sets.  -> a SetList: summarize()'s dict per set, bit for bit what summarize returns
    for the set's rows alone, or None for a set without an included row of positive weight (`failed` {set: message})."""
    return _summarize(cols, set_start, weights, nbins, pairs, pair_bins, device)


# ---- chain pools ------------------------------------------------------------------------------------------

def pool_columns(pool, ci, ri, moho=None, mohovs=4.2, device=None):
    """The scalar parameters of the pool's rows (ci, ri) as Columns on the device, named NAMES(...), each in the dtype
    save() writes it in; the layer count from the model rows (Plotting.py:612-613); with moho = (zlo, zhi) the Moho
    depth of every row as moho.py derives it (bh_moho_rows on the widened rows), NaN without one."""
    import torch
    from . import moho as mh
    nt = pool.ntargets
    refs = [t.ref for t in pool.targets.targets]
    models = pool.models[ci, ri]
    host = np.empty((ci.size, 3 * nt + 4 + (moho is not None)))
    host[:, 0] = pool.likes[ci, ri]
    host[:, 1:nt + 2] = pool.misfits[ci, ri]
    host[:, nt + 2] = pool.vpvs[ci, ri]
    host[:, nt + 3:3 * nt + 3] = pool.noise[ci, ri]
    host[:, 3 * nt + 3] = (~np.isnan(models)).sum(axis=1) / 2 - 1
    dev = _device.torch_device(device)
    M = _device.to_device(host, torch.float64, dev)
    if moho is not None and ci.size:
        zlo, zhi, mohovs, _ = mh._window(moho, mohovs, 1)
        with torch.cuda.device(dev):
            D = mh.derive(mh._widened(models, dev), zlo, zhi, mohovs, torch.cuda.current_stream(dev).cuda_stream)
            M[:, -1] = D[:, 0]
    return Columns(M, TAGS(nt, moho is not None), NAMES(nt, refs, moho is not None))


def pool_scalars(pool, selection='weighted', dev=0.05, exclude_outliers=True, nbins=20, pairs=(), pair_bins=50, moho=None,
                 mohovs=4.2, by_chain=False, device=None):
    """ChainPool.scalars: summarize() over the rows ChainPool.posterior uses, plus 'chains' (global indices used); with
    by_chain one set per chain (summarize_sets; chains are contiguous in the selection's order)."""
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    cols = pool_columns(pool, ci, ri, moho, mohovs, device)
    if by_chain:
        res = summarize_sets(cols, np.searchsorted(ci, np.arange(pool.nchains + 1)), w.astype(np.int32), nbins, pairs,
                             pair_bins, device)
        res.chains = np.unique(ci) + pool.first
        return res
    res = summarize(cols, w.astype(np.int32), nbins, pairs, pair_bins, device)
    res['chains'] = np.unique(ci) + pool.first
    return res


# ---- station pools ------------------------------------------------------------------------------------------

def _stack(values, shape=()):
    """Per-station values (None: a station without) -> one float64 array, NaN where there is none; arrays of different
    lengths (the bins of a count or of a constant) are filled up with NaN."""
    have = [np.asarray(v, dtype=np.float64) for v in values if v is not None]
    tail = tuple(max([h.shape[i] for h in have] + [0]) for i in range(len(shape))) if shape else ()
    out = np.full((len(values),) + tail, np.nan)
    for z, v in enumerate(values):
        if v is not None:
            v = np.asarray(v, dtype=np.float64)
            out[(z,) + tuple(slice(0, n) for n in v.shape)] = v
    return out


class StationScalars(sel.StationResult):
    """StationPool.scalars' result, every array in the pool's station order.

    names, failed    the stations; {station name: message} (such a station is a row of NaN)
    stations         {station name: the dict pool.station(name).scalars(...) returns}, failed stations left out
    columns          the names of the columns with statistics (scalars.NAMES)
    nmodels, nexcluded [nstations]; with moho also nmodels_moho, nexcluded_moho
    stats            {column: dict(median, mean, std, min, max, mode, constant [nstations], hist [nstations, bins],
                     edges [nstations, bins + 1])} -- bins = nbins; where the bins of a column differ between stations
                     (the layer count, a constant) the shorter rows are filled up with NaN
    pairs            {(x, y): dict(counts [nstations, pb, pb], xedges, yedges [nstations, pb + 1], mode [nstations, 2])}"""

    FIELDS = ('median', 'mean', 'std', 'min', 'max', 'mode', 'constant')

    def __init__(self, names, results, failed):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {n: r for n, r in zip(names, results) if r is not None}
        first = next((r for r in results if r is not None), None)
        get = lambda key, sub=None: [None if r is None else (r[key] if sub is None else r[key][sub]) for r in results]
        self.columns = [] if first is None else [k for k, v in first.items() if isinstance(v, dict) and k != 'pairs']
        for k in ([] if first is None else [k for k in first if k.startswith('nmodels') or k.startswith('nexcluded')]):
            setattr(self, k, np.array([0 if v is None else v for v in get(k)], dtype=np.int64))
        self.stats, self.pairs = {}, {}
        for c in self.columns:
            d = {k: _stack(get(c, k)) for k in self.FIELDS}
            d['hist'] = _stack([None if r is None else r[c]['hist'][0] for r in results], (0,))
            d['edges'] = _stack([None if r is None else r[c]['hist'][1] for r in results], (0,))
            self.stats[c] = d
        for p in ([] if first is None else first['pairs']):
            rec = lambda k: [None if r is None else r['pairs'][p][k] for r in results]
            self.pairs[p] = dict(counts=_stack(rec('counts'), (0, 0)), xedges=_stack(rec('xedges'), (0,)),
                                 yedges=_stack(rec('yedges'), (0,)), mode=_stack(rec('mode'), (0,)))


def stations_scalars(spool, selection='weighted', dev=0.05, exclude_outliers=True, nbins=20, pairs=(), pair_bins=50,
                     moho=None, mohovs=4.2, device=None, strict=True, max_rows=None):
    """StationPool.scalars: summarize_sets() over every station's main-phase rows (see StationPool.scalars)."""
    import torch
    pool, c = spool.pool, spool.chains_per_station
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    if max_rows is None:       # half of the free device memory: the matrix, and with moho the widened model rows
        per_row = 8 * (3 * pool.ntargets + 5) + (12 * pool.models.shape[2] + 32 if moho is not None else 0)
        max_rows = max(1, int(torch.cuda.mem_get_info(_device.torch_device(device))[0] // (2 * per_row)))
    results = []
    for a, b in df.station_runs(set_start, max_rows):
        lo, hi = int(set_start[a]), int(set_start[b])
        cols = pool_columns(pool, ci[lo:hi], ri[lo:hi], moho, mohovs, device)
        res = summarize_sets(cols, set_start[a:b + 1] - lo, w[lo:hi].astype(np.int32), nbins, pairs, pair_bins, device)
        results += list(res)
        for z, msg in res.failed.items():
            failed.setdefault(a + z, msg)
    sel.raise_first_failed(failed, strict, "station", spool.names)
    for z, r in enumerate(results):
        if r is not None:
            r['chains'] = sel.station_chains(ci, set_start, z, c)
    return StationScalars(spool.names, results, failed)
