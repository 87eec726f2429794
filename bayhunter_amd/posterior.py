"""Velocity-depth posterior of a block of sampled models, on the device (include/bayhunter_amd.h, bh_posterior_*).

What the reference computes after an inversion, from the rows of the main phase:

    ModelMatrix.get_singlemodels(models, dep_int, misfits)   src/Models.py:160-226   mean, median, minmax,
                                                                                    stdminmax, mode, minmisfit
    PlotFromStorage._plot_bestmodels_hist(models, dep_int)   src/Plotting.py:462-536 the Vs-depth density and
                                                                                    the interface-depth histogram
    PlotFromStorage.plot_posterior_nlayers                   src/Plotting.py:607-625 the layer-count histogram

Every row carries an integer weight (the iterations it stayed current); the result equals the reference's on
the matrix in which each row is repeated `weight` times, without building that matrix.  Edge arrays are made
here with numpy exactly as the reference makes them; the device bins by binary search over them.
"""
import ctypes as C

import numpy as np

from . import _device, _lib, selection as sel      # (`selection` is a parameter of the entry points)

VS_INTERVAL = 0.025          # km/s: the reference's Vs bin width (Models.py:204, Plotting.py:495)


def default_dep_int():
    """get_singlemodels' default grid: 0.5 km steps to 100 km."""
    return np.linspace(0, 100, 201)


def models2d_dep_int(z, depint=1):
    """The grid plot_posterior_models2d passes (Plotting.py:741-742): arange(z0, z1 + depint, depint)."""
    return np.arange(z[0], z[1] + depint, depint)


def hist_grids(dep_int=None):
    """(half-step depth grid, depth bin edges) of _plot_bestmodels_hist (Plotting.py:470-480)."""
    if dep_int is None:
        return np.linspace(0, 100, 201), np.linspace(0, 100, 101)
    dep_int = np.asarray(dep_int, dtype=np.float64)
    maxdepth = int(np.ceil(dep_int.max()))
    interp = dep_int[1] - dep_int[0]
    return (np.arange(dep_int[0], dep_int[-1] + interp / 2., interp / 2.),
            np.arange(0, maxdepth + 2 * interp, interp))


def vs_round(vs):
    """Plotting.py:29-33: rounds to the nearest 0.025 km/s."""
    vs_floor = np.floor(vs)
    return np.round((vs - vs_floor) * 40) / 40 + vs_floor


def bin_index(values, edges):
    """Bin of each value, -1 outside: edges[i] <= v < edges[i+1], the last bin closed (numpy's histogram rule)."""
    values, edges = np.asarray(values, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    i = np.searchsorted(edges, values, side='right') - 1
    i[values == edges[-1]] = edges.size - 2
    i[(i < 0) | (i > edges.size - 2)] = -1
    return i.astype(np.int32)


def stepmodel(row):
    """Model.get_stepmodel (Models.py:55-70) of one row: (vs_step, dep_step)."""
    model = np.asarray(row, dtype=np.float64)
    model = model[~np.isnan(model)]
    n = int(model.size / 2)
    vs, z = model[:n], model[-n:]
    z_disc = (z[:n - 1] + z[1:n]) / 2.
    h = np.concatenate((z_disc - np.concatenate(([0], z_disc[:-1])), [0]))
    dep = np.cumsum(h)
    dep = np.concatenate([(d, d) for d in dep])
    dep_step = np.concatenate([[0], dep[:-1]])
    vs_step = np.concatenate([(v, v) for v in vs])
    dep_step[-1] = np.max([150, dep_step[-1] * 2.5])
    return vs_step, dep_step


class Grid(_device.Handle):
    """One bh_posterior handle: the rows on one depth grid."""

    def __init__(self, rows, weights, misfits, dep, ifedges, stream):
        self.dep = np.ascontiguousarray(dep, dtype=np.float64)
        self.ifedges = None if ifedges is None else np.ascontiguousarray(ifedges, dtype=np.float64)
        self.width = rows.shape[1]
        nif = 0 if self.ifedges is None else self.ifedges.size
        _device.Handle.__init__(
            self, 'posterior', rows.data_ptr(), int(rows.dtype.itemsize == 8), rows.shape[0], rows.stride(0),
            self.width, None if weights is None else weights.data_ptr(),
            None if misfits is None else misfits.data_ptr(), self.dep.ctypes.data, self.dep.size,
            None if not nif else self.ifedges.ctypes.data, nif, stream)

    def scan(self):
        D = self.dep.size
        total, argmin = C.c_longlong(0), C.c_longlong(-1)
        vmin, vmax, mean = np.zeros(D), np.zeros(D), np.zeros(D)
        nlay = np.zeros(self.width // 2 + 1, dtype=np.int64)
        ifh = np.zeros(max(0, (0 if self.ifedges is None else self.ifedges.size) - 1), dtype=np.int64)
        _lib.check(self.lib.bh_posterior_scan(self.h, C.byref(total), vmin.ctypes.data, vmax.ctypes.data,
                                              mean.ctypes.data, nlay.ctypes.data,
                                              ifh.ctypes.data if ifh.size else None, C.byref(argmin)))
        return dict(total=total.value, vmin=vmin, vmax=vmax, mean=mean, nlayers=nlay, ifhist=ifh, argmin=argmin.value)

    def finish(self, vedges, dbin, ndbins, stats):
        D = self.dep.size
        vedges = np.ascontiguousarray(vedges, dtype=np.float64)
        dbin = np.ascontiguousarray(dbin, dtype=np.int32)
        hist = np.zeros((ndbins, vedges.size - 1), dtype=np.int64)
        std, median = (np.zeros(D), np.zeros(D)) if stats else (None, None)
        _lib.check(self.lib.bh_posterior_finish(self.h, vedges.ctypes.data, vedges.size, dbin.ctypes.data, ndbins,
                                                hist.ctypes.data, None if std is None else std.ctypes.data,
                                                None if median is None else median.ctypes.data))
        return hist, std, median


def _grids(dep_int, depint):
    """(depth grid of the single models, half-step grid and depth bin edges of the density) as summarize takes them."""
    hist_dep_int = dep_int
    if dep_int is None and depint is not None:
        dep_int = hist_dep_int = models2d_dep_int((0, 100), depint)
    dep_int = default_dep_int() if dep_int is None else np.asarray(dep_int, dtype=np.float64)
    dep2, depbins = hist_grids(hist_dep_int)
    if dep_int.size < 2:
        raise ValueError("dep_int: at least two depths (they are the mode histogram's depth edges)")
    return dep_int, dep2, depbins


def mode_edges(vmin, vmax):
    """Vs edges of get_singlemodels' mode histogram, from the per-depth min / max of a scan: int((max - min) / 0.025)
    bins over linspace(min, max).  ValueError where the reference raises (no bin)."""
    vmin, vmax = vmin.min(), vmax.max()
    vsbins = int((vmax - vmin) / VS_INTERVAL)
    if vsbins < 1:
        raise ValueError("`bins[0]` must be positive, when an integer (all Vs values within 0.025 km/s)")
    return np.linspace(vmin, vmax, vsbins + 1)


def density_edges(vmin, vmax):
    """Vs edges of _plot_bestmodels_hist, from the per-depth min / max of a scan on its half-step grid."""
    vmin, vmax = vmin.min(), vmax.max()
    return np.arange(vs_round(vmin) - 2 * VS_INTERVAL, vs_round(vmax) + 3 * VS_INTERVAL, VS_INTERVAL)


def _result(s, dep_int, vedges, mhist, std, median, h2, vsb, depbins, minmisfit):
    """summarize()'s dict from a scan `s` (total, vmin, vmax, mean, nlayers, ifhist), the finish on both grids and
    the row of the least misfit (None: no misfits)."""
    mean = s['mean']
    vs_center = (vedges[:-1] + vedges[1:]) / 2.
    dep_center = (dep_int[:-1] + dep_int[1:]) / 2.
    single = dict(mean=(mean, dep_int), median=(median, dep_int),
                  minmax=(np.array((s['vmin'], s['vmax'])), dep_int),
                  stdminmax=(np.array((mean - std, mean + std)), dep_int),
                  mode=(vs_center[np.argmax(mhist, axis=1)], dep_center))
    if minmisfit is not None:
        single['minmisfit'] = stepmodel(minmisfit)
    return dict(singlemodels=single, hist2d=(h2.T.copy(), vsb, depbins), interfaces=(s['ifhist'], depbins),
                nlayers=s['nlayers'], nmodels=s['total'])


def summarize(models, weights=None, dep_int=None, misfits=None, depint=None, device=None):
    """Posterior statistics of `models` ([rows, 2*maxlayers], reference layout, float32 or float64; numpy or
    a torch tensor) with integer `weights` (>= 0, default 1 each).

    dep_int   depth grid of get_singlemodels and _plot_bestmodels_hist (default: their own defaults).  With
              `depint` and no dep_int: plot_posterior_models2d's grid arange(0, 100 + depint, depint).
    misfits   one value per row: singlemodels['minmisfit'] is the step model of the first least misfit.

    -> dict(singlemodels = get_singlemodels(models, dep_int, misfits),
            hist2d       = (counts[vs bin, depth bin], vs edges, depth edges)  as np.histogram2d returns them,
            interfaces   = (counts, depth edges)  of the interface depths,
            nlayers      = counts by number of nuclei n (index n; plot_posterior_nlayers shows n - 1 layers),
            nmodels      = the weighted number of models (the reference's "%d models"))
    ValueError where the reference raises (all values equal: no mode bin) and for an empty selection."""
    import torch
    dev, rows, w, mf = _device.device_rows(models, weights, misfits, device)
    if rows.shape[0] == 0:
        raise ValueError("empty selection: no models")
    dep_int, dep2, depbins = _grids(dep_int, depint)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        with Grid(rows, w, mf, dep_int, depbins, stream) as ga:
            s = ga.scan()
            vedges = mode_edges(s['vmin'], s['vmax'])
            mhist, std, median = ga.finish(vedges, bin_index(dep_int, dep_int), dep_int.size - 1, True)
        # the density of _plot_bestmodels_hist on its half-step grid
        with Grid(rows, w, None, dep2, None, stream) as gb:
            s2 = gb.scan()
            vsb = density_edges(s2['vmin'], s2['vmax'])
            h2, _, _ = gb.finish(vsb, bin_index(dep2, depbins), depbins.size - 1, False)
    minmisfit = None if mf is None else rows[s['argmin']].cpu().numpy()
    return _result(s, dep_int, vedges, mhist, std, median, h2, vsb, depbins, minmisfit)


# ---- many sets of rows in one pass ------------------------------------------------------------------------

class Sets(_device.Handle):
    """One bh_posterior_sets handle: the rows, in contiguous sets, on one depth grid."""

    def __init__(self, rows, weights, misfits, set_start, dep, ifedges, stream, chunk_bytes=None):
        self.dep = np.ascontiguousarray(dep, dtype=np.float64)
        self.ifedges = None if ifedges is None else np.ascontiguousarray(ifedges, dtype=np.float64)
        self.set_start = np.ascontiguousarray(set_start, dtype=np.int64)
        self.width, self.nsets = rows.shape[1], self.set_start.size - 1
        nif = 0 if self.ifedges is None else self.ifedges.size
        _device.Handle.__init__(
            self, 'posterior_sets', rows.data_ptr(), int(rows.dtype.itemsize == 8), rows.shape[0], rows.stride(0),
            self.width, None if weights is None else weights.data_ptr(),
            None if misfits is None else misfits.data_ptr(), self.set_start.ctypes.data, self.nsets,
            self.dep.ctypes.data, self.dep.size, None if not nif else self.ifedges.ctypes.data, nif, stream)
        if chunk_bytes is not None:
            _lib.check(self.lib.bh_posterior_sets_set_chunk_bytes(self.h, int(chunk_bytes)))

    def scan(self):
        """-> dict of arrays with one row per set, and 'status' (0: the set has statistics)."""
        S, D = self.nsets, self.dep.size
        total, argmin = np.zeros(S, dtype=np.int64), np.full(S, -1, dtype=np.int64)
        status = np.zeros(S, dtype=np.int32)
        vmin, vmax, mean = np.zeros((S, D)), np.zeros((S, D)), np.zeros((S, D))
        nlay = np.zeros((S, self.width // 2 + 1), dtype=np.int64)
        ifh = np.zeros((S, max(0, (0 if self.ifedges is None else self.ifedges.size) - 1)), dtype=np.int64)
        _lib.check(self.lib.bh_posterior_sets_scan(self.h, total.ctypes.data, vmin.ctypes.data, vmax.ctypes.data,
                                                   mean.ctypes.data, nlay.ctypes.data,
                                                   ifh.ctypes.data if ifh.size else None, argmin.ctypes.data,
                                                   status.ctypes.data))
        return dict(total=total, vmin=vmin, vmax=vmax, mean=mean, nlayers=nlay, ifhist=ifh, argmin=argmin,
                    status=status)

    def finish(self, vedges, dbin, ndbins, stats):
        """vedges: per set its Vs edges, or None to leave the set out -> (per set hist[ndbins, edges - 1] or None,
        std [sets, D], median [sets, D]) -- the last two None without `stats`, NaN rows for sets left out."""
        S, D = self.nsets, self.dep.size
        nve = np.array([0 if e is None else e.size for e in vedges], dtype=np.int64)
        off = np.concatenate(([0], np.cumsum(nve))).astype(np.int32)
        allv = np.ascontiguousarray(np.concatenate([e for e in vedges if e is not None] + [np.zeros(1)]))
        hoff = np.concatenate(([0], np.cumsum(ndbins * np.maximum(nve - 1, 0))))
        dbin = np.ascontiguousarray(dbin, dtype=np.int32)
        hist = np.zeros(max(1, hoff[-1]), dtype=np.int64)
        std, median = (np.zeros((S, D)), np.zeros((S, D))) if stats else (None, None)
        _lib.check(self.lib.bh_posterior_sets_finish(self.h, allv.ctypes.data, off.ctypes.data, dbin.ctypes.data, ndbins,
                                                     hist.ctypes.data, None if std is None else std.ctypes.data,
                                                     None if median is None else median.ctypes.data))
        hists = [None if vedges[z] is None else hist[hoff[z]:hoff[z + 1]].reshape(ndbins, nve[z] - 1) for z in range(S)]
        return hists, std, median


class SetResults(sel.SetList):
    """summarize_sets' list: entry s is summarize()'s dict of set s, or None for a set in `failed`
    ({set index: message}).  `std[s]` is the set's standard deviation per depth (summarize reports mean -+ std)."""

    def __init__(self, results, failed, dep_int, std):
        sel.SetList.__init__(self, results, failed)
        self.dep, self.std = dep_int, std

    def section(self):
        """The single models stacked: dict(dep [D], mean / median / std / vmin / vmax [sets, D], mode [sets, D - 1]),
        a failed set a row of NaN."""
        S, D = len(self), self.dep.size
        out = dict(dep=self.dep)
        for k in ('mean', 'median', 'std', 'vmin', 'vmax'):
            out[k] = np.full((S, D), np.nan)
        out['mode'] = np.full((S, D - 1), np.nan)
        for z, res in enumerate(self):
            if res is None:
                continue
            sm = res['singlemodels']
            out['mean'][z], out['median'][z], out['std'][z] = sm['mean'][0], sm['median'][0], self.std[z]
            out['vmin'][z], out['vmax'][z] = sm['minmax'][0]
            out['mode'][z] = sm['mode'][0]
        return out


def summarize_sets(models, set_start, weights=None, dep_int=None, misfits=None, depint=None, device=None, strict=True,
                   chunk_bytes=None):
    """summarize() of every set of rows in one pass: set s is models[set_start[s]:set_start[s + 1]] (set_start
    [sets + 1], ascending from 0 to the number of rows; a set may be empty), with its weights and misfits.

    -> SetResults: a list with summarize()'s dict per set, every field bit for bit what summarize returns for the
    set's rows alone.  A set for which summarize raises (empty selection; all Vs within 0.025 km/s) raises here
    too, as a ValueError naming the first such set -- or, with strict=False, has the entry None and its message in
    the list's `failed` {set index: message}.  A negative weight fails the call.

    chunk_bytes   bound on the device memory of the median's digit table (default 64 MiB): the sets are processed
                  in chunks that keep to it, and no result depends on it."""
    import torch
    dev, rows, w, mf = _device.device_rows(models, weights, misfits, device)
    set_start, S = sel.check_set_start(set_start, rows.shape[0])
    dep_int, dep2, depbins = _grids(dep_int, depint)
    failed, results, std = {}, [None] * S, None
    if rows.shape[0] == 0:
        failed = {z: "empty selection: no models" for z in range(S)}
    else:
        lib = _lib.load()
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            with Sets(rows, w, mf, set_start, dep_int, depbins, stream, chunk_bytes) as ga:
                s = ga.scan()
                vedges = [None] * S
                for z in range(S):
                    if s['status'][z]:
                        failed[z] = lib.bh_posterior_sets_status_text(int(s['status'][z])).decode()
                        continue
                    try:
                        vedges[z] = mode_edges(s['vmin'][z], s['vmax'][z])
                    except ValueError as e:
                        failed[z] = str(e)
                mhist, std, median = ga.finish(vedges, bin_index(dep_int, dep_int), dep_int.size - 1, True)
            with Sets(rows, w, None, set_start, dep2, None, stream, chunk_bytes) as gb:
                s2 = gb.scan()
                vsb = [None if z in failed else density_edges(s2['vmin'][z], s2['vmax'][z]) for z in range(S)]
                h2, _, _ = gb.finish(vsb, bin_index(dep2, depbins), depbins.size - 1, False)
        live = [z for z in range(S) if z not in failed]
        best = None if mf is None or not live else rows[torch.from_numpy(s['argmin'][live]).to(dev)].cpu().numpy()
        for i, z in enumerate(live):
            sz = {k: s[k][z] for k in ('vmin', 'vmax', 'mean', 'nlayers', 'ifhist')}
            sz['total'] = int(s['total'][z])
            results[z] = _result(sz, dep_int, vedges[z], mhist[z], std[z], median[z], h2[z], vsb[z], depbins,
                                 None if best is None else best[i])
    sel.raise_first_failed(failed, strict, "set")
    return SetResults(results, failed, dep_int, std)


# ---- the chain pool's own sample block, and every station of a station pool --------------------------------

def pool_posterior(pool, dep_int=None, depint=1, dev=0.05, exclude_outliers=True, selection='weighted', device=None):
    """ChainPool.posterior: summarize() over the pool's main-phase rows (see ChainPool.posterior)."""
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    if dep_int is None:
        dep_int = models2d_dep_int(pool.priors['z'], depint)
    res = summarize(pool.models[ci, ri], w.astype(np.int32), dep_int=dep_int, device=device)
    res['chains'] = np.unique(ci) + pool.first
    return res


class StationPosterior(sel.StationResult):
    """StationPool.posterior's result.

    stations   {station name: the dict pool.station(name).posterior(...) returns}, failed stations left out
    failed     {station name: message}
    dep        the depth grid [D]
    mean, median, std, vmin, vmax [nstations, D], mode [nstations, D - 1]   the single models of all stations, in
               the pool's station order: the section (or, with the stations' coordinates, the volume); a failed
               station is a row of NaN"""

    def __init__(self, names, results, failed):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {n: r for n, r in zip(names, results) if r is not None}
        for k, v in results.section().items():
            setattr(self, k, v)


def stations_posterior(spool, dep_int=None, depint=1, dev=0.05, exclude_outliers=True, selection='weighted', device=None,
                       strict=True):
    """StationPool.posterior: summarize_sets() over every station's main-phase rows (see StationPool.posterior)."""
    pool, c = spool.pool, spool.chains_per_station
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    if dep_int is None:
        dep_int = models2d_dep_int(pool.priors['z'], depint)
    res = summarize_sets(pool.models[ci, ri], set_start, w.astype(np.int32), dep_int=dep_int, device=device, strict=False)
    res.failed.update(failed)
    sel.raise_first_failed(res.failed, strict, "station", spool.names)
    for z, r in enumerate(res):
        if r is not None:
            r['chains'] = sel.station_chains(ci, set_start, z, c)
    return StationPosterior(spool.names, res, res.failed)
