"""Posterior statistics of the modelled data, on the device (include/bayhunter_amd.h, bh_datafits_*).

The reference looks at the data fit of an inversion one model per chain (PlotFromStorage.plot_bestdatafits,
src/Plotting.py:1054-1111; plot_rfcorr, :1114-1150): the least-misfit saved model of each chain through
target.moddata.plugin.run_model.  Here every sampled row goes through the batched forward pass
(models.layers_from_voronoi -> ForwardEngine.run, into one device matrix) and the library reduces every
column of that matrix over the weighted rows: mean, std, min, max, exact percentiles and a histogram per
sample (the "data fan"), as on the matrix in which every row is repeated `weight` times.

Rows whose forward pass failed (a dispersion search that found no root) or whose modelled data hold a NaN
are left out and counted (`nexcluded`, in weighted rows).

The stations of a network (StationPool) are summarised in one pass: summarize_sets / stations_datafits put the rows
of all stations through one forward pass and one segmented reduction (bh_datafits_sets_*), per station bit for bit
what summarize gives for the station's rows alone.
"""
import ctypes as C

import numpy as np

from . import _device, _lib, selection as sel      # (`selection` is a parameter of the entry points)

DEFAULT_Q = (2.5, 16, 50, 84, 97.5)
CHUNK = 65536                     # rows per layers_from_voronoi call: bounds the packed-model temporaries
_OPEN_PRIORS = dict(layers=(0, 1 << 30), vs=(-np.inf, np.inf), z=(-np.inf, np.inf))   # valid flags unused


def percentile_ranks(q, W):
    """0-based ranks into the expanded column that numpy's default ('linear') percentile of `q` reads, with
    numpy interpolates between: (virtual index, lower rank, upper rank) per q."""
    q = np.asarray(q, dtype=np.float64)
    if q.ndim != 1 or np.any(q < 0) or np.any(q > 100) or np.any(np.isnan(q)):
        raise ValueError("q: percentiles in [0, 100]")
    virt = np.true_divide(q, 100) * (W - 1)
    lo = np.floor(virt)
    hi = np.ceil(virt)           # method='higher'; equals lo where t = 0
    return virt, lo.astype(np.int64), hi.astype(np.int64)


def lerp(a, b, t):
    """numpy's _lerp (numpy/lib/_function_base_impl.py): a + (b - a) t, from the upper end for t >= 0.5."""
    d = b - a
    out = a + d * t
    return np.where(t >= 0.5, b - d * (1 - t), out)


def _layers(models, dev):
    """Reference-layout rows (fp64 device tensor) -> (VSN, ZV, nlay) of layers_from_voronoi."""
    import torch
    R, Wd = models.shape
    maxn = Wd // 2
    cnt = (~torch.isnan(models)).sum(dim=1)
    n = (cnt // 2).to(torch.int64)
    k = torch.arange(maxn, device=dev)[None, :]
    have = k < n[:, None]
    vsn = torch.where(have, models[:, :maxn], torch.zeros((), dtype=models.dtype, device=dev))
    zi = torch.clamp(n[:, None] + k, max=Wd - 1)
    zv = torch.where(have, torch.gather(models, 1, zi), torch.zeros((), dtype=models.dtype, device=dev))
    return vsn.contiguous(), zv.contiguous(), n.to(torch.int32)


class Fits(_device.Handle):
    """One bh_datafits handle over a device matrix."""

    def __init__(self, Y, ncols, weights, err, stream):
        self.ncols = ncols
        _device.Handle.__init__(
            self, 'datafits', Y.data_ptr(), Y.shape[0], Y.stride(0), ncols, None if weights is None else
            weights.data_ptr(), None if err is None else err.data_ptr(), 0 if err is None else err.shape[1], stream)

    def scan(self):
        N = self.ncols
        total, excl = C.c_longlong(0), C.c_longlong(0)
        vmin, vmax, mean = np.zeros(N), np.zeros(N), np.zeros(N)
        _lib.check(self.lib.bh_datafits_scan(self.h, C.byref(total), C.byref(excl), vmin.ctypes.data,
                                             vmax.ctypes.data, mean.ctypes.data))
        return dict(total=total.value, excluded=excl.value, vmin=vmin, vmax=vmax, mean=mean)

    def finish(self, ranks, edges, eset):
        N = self.ncols
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        eset = np.ascontiguousarray(eset, dtype=np.int32)
        ost = np.zeros((ranks.size, N))
        hist = np.zeros((N, edges.shape[1] - 1), dtype=np.int64)
        std = np.zeros(N)
        _lib.check(self.lib.bh_datafits_finish(
            self.h, ranks.ctypes.data if ranks.size else None, ranks.size, ost.ctypes.data if ranks.size else None,
            edges.ctypes.data, edges.shape[1], edges.shape[0], eset.ctypes.data, hist.ctypes.data, std.ctypes.data))
        return ost, hist, std


def forward_matrix(targets, models, vpvs, mantle=None, device=None, rf_p=None, set_id=None):
    """The modelled data of every row on the device -> (engine, Y [rows, engine.row] fp64, err [rows, nflags],
    batch layout).  Layers: layers_from_voronoi (Model.get_vp_vs_h, rho = 0.77 + 0.32 vp) in chunks.

    rf_p, set_id   rows of several stations in one matrix: rf_p [nstations, nrf] (stations.rf_slowness_table) and the
                   station of every row, set_id [rows]; every row's receiver functions are then computed at its own
                   station's ray parameter (ForwardEngine.run's rf_sets), bit for bit the row of that station's engine."""
    import torch
    from .engine import ForwardEngine
    from .models import layers_from_voronoi
    dev = _device.torch_device(device)
    bl = targets.batch_layout(ell=True)
    lay = bl['layout']
    with torch.cuda.device(dev):
        # ell_flags: a row without an ellipticity is flagged, and left out, like a row whose search failed
        eng = ForwardEngine(swd=lay.swd, rf=lay.rf, device=dev, ell=lay.ell, ell_flags=True)
        rows = _device.to_device(models, torch.float64, dev)
        vpvs = _device.to_device(np.broadcast_to(np.asarray(vpvs, dtype=np.float64), (rows.shape[0],))
                                 if not isinstance(vpvs, torch.Tensor) else vpvs, torch.float64, dev)
        R = rows.shape[0]
        tab = ids = None
        if rf_p is not None and lay.rf:
            rf_p = np.asarray(rf_p, dtype=np.float64)
            if rf_p.ndim != 2 or rf_p.shape[1] != len(lay.rf) or set_id is None or len(set_id) != R:
                raise ValueError("rf_p: [nstations, %d receiver functions], with one station index per row" % len(lay.rf))
            tab = _device.to_device(np.ascontiguousarray(rf_p.T), torch.float64, dev)
            ids = _device.to_device(set_id, torch.int32, dev)
        need = R * eng.row * 8 + R * bl['nflags'] * 4
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise ValueError("the modelled data of %d rows need %.1f GB of device memory, %.1f GB are free: use "
                             "selection='saved' (the thinned rows save() writes)" % (R, need / 1e9, free / 1e9))
        Y, err = eng.alloc_out(R)
        for lo in range(0, R, CHUNK):
            hi = min(R, lo + CHUNK)
            vsn, zv, nl = _layers(rows[lo:hi], dev)
            dm, _ = layers_from_voronoi(vsn, zv, nl, vpvs[lo:hi], _OPEN_PRIORS, mantle=mantle, device=dev)
            eng.run(dm, out=Y[lo:hi], err=err[lo:hi], rf_sets=None if tab is None else (tab, ids[lo:hi]))
    return eng, Y, err, bl


def order_ranks(q, W):
    """The order statistics the percentiles `q` and the median of a column of weight total W are made of
    -> (virt, lo, hi, med, ranks): percentile_ranks(q, W), the two middle ranks, and all of them sorted and distinct."""
    virt, lo, hi = percentile_ranks(q, W)
    med = np.array([(W - 1) // 2, W // 2], dtype=np.int64)
    ranks = np.unique(np.concatenate((lo, hi, med)))
    if ranks.size > _lib.MAX_DATAFITS_RANKS:
        raise ValueError("too many percentiles: at most %d distinct order statistics" % _lib.MAX_DATAFITS_RANKS)
    return virt, lo, hi, med, ranks


def target_edges(vmin, vmax, segs, nbins):
    """Histogram edges per target from the per-column min / max of a scan: nbins bins over the target's range
    (+- 0.5 when it is a point) -> (edges [targets, nbins + 1], eset [columns]: the target of every column)."""
    eset = np.zeros(len(vmin), dtype=np.int32)
    edges = np.zeros((len(segs), int(nbins) + 1))
    for t, (a, b) in enumerate(segs):
        tmin, tmax = vmin[a:b].min(), vmax[a:b].max()
        if tmin == tmax:
            tmin, tmax = tmin - 0.5, tmax + 0.5
        edges[t] = np.linspace(tmin, tmax, int(nbins) + 1)
        eset[a:b] = t
    return edges, eset


def _result(targets, segs, s, rk, ost, hist, std, edges, best, q):
    """summarize()'s dict from a scan `s` (total, excluded, vmin, vmax, mean), order_ranks' tuple `rk`, the finish
    (order statistics of rk's ranks, histograms, std) and the best row (None: no misfits)."""
    virt, lo, hi, med, ranks = rk
    at = {r: i for i, r in enumerate(ranks.tolist())}
    vlo, vhi = ost[[at[r] for r in lo]], ost[[at[r] for r in hi]]
    t = (virt - lo)[:, None]
    quant = lerp(vlo, vhi, t)
    median = (ost[at[int(med[0])]] + ost[at[int(med[1])]]) / 2.
    out = []
    for n, (a, b) in enumerate(segs):
        tg = targets.targets[n]
        d = dict(ref=tg.ref, x=np.asarray(tg.obsdata.x), yobs=np.asarray(tg.obsdata.y),
                 mean=s['mean'][a:b], std=std[a:b], min=s['vmin'][a:b], max=s['vmax'][a:b], median=median[a:b],
                 quantiles=quant[:, a:b], density=(hist[a:b], edges[n]))
        if best is not None:
            d['best'] = best[a:b]
            d['residual'] = d['yobs'] - d['best']
        out.append(d)
    return dict(targets=out, q=np.asarray(q, dtype=np.float64), nmodels=s['total'], nexcluded=s['excluded'])


def _summarize(targets, models, vpvs, weights, misfits, mantle, q, nbins, device, pick=None):
    import torch
    dev = _device.torch_device(device)
    if not isinstance(models, torch.Tensor):
        models = np.asarray(models)
    if models.ndim != 2 or models.shape[0] == 0:
        raise ValueError("models: [rows, 2*maxlayers], at least one row")
    R = models.shape[0]
    if int(nbins) < 1:
        raise ValueError("nbins >= 1")
    w = None if weights is None else _device.to_device(weights, torch.int32, dev)
    if w is not None and w.numel() != R or misfits is not None and np.asarray(misfits).size != R:
        raise ValueError("one weight and one misfit per row")
    eng, Y, err, bl = forward_matrix(targets, models, vpvs, mantle, dev)
    desc = bl['desc']
    segs = [(desc[n].off, desc[n].off + desc[n].n) for n in range(targets.ntargets)]
    ncols = eng.ncols
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        with Fits(Y, ncols, w, err, stream) as f:
            s = f.scan()
            rk = order_ranks(q, s['total'])
            edges, eset = target_edges(s['vmin'], s['vmax'], segs, nbins)
            ost, hist, std = f.finish(rk[4], edges, eset)
        picked = None if pick is None else Y[torch.as_tensor(np.asarray(pick, dtype=np.int64), device=dev)].cpu().numpy()
        best = None
        if misfits is not None:
            mf = np.asarray(misfits, dtype=np.float64)
            wh = np.ones(R, dtype=bool) if weights is None else np.asarray(
                weights.cpu().numpy() if isinstance(weights, torch.Tensor) else weights) > 0
            cand = np.nonzero(wh)[0]
            best = Y[int(cand[np.argmin(mf[cand])])].cpu().numpy()
    res = _result(targets, segs, s, rk, ost, hist, std, edges, best, q)
    if pick is not None:
        res['_picked'] = [picked[:, a:b] for a, b in segs]
    return res


def summarize(targets, models, vpvs, weights=None, misfits=None, mantle=None, q=DEFAULT_Q, nbins=100, device=None):
    """Statistics of the modelled data of `models` ([rows, 2*maxlayers], reference layout, float32 / float64, numpy
    or torch) with vp/vs `vpvs` (one per row, or a scalar), integer `weights` (>= 0, default 1 each) and the
    prior's `mantle` (vs, vpvs) rule, for every target of the JointTarget `targets`.

    -> dict(targets = [per target, in JointTarget order: dict(ref, x, yobs, mean, std, min, max, median,
                        quantiles [len(q), S] (numpy's 'linear' percentiles), density = (counts [S, nbins],
                        edges over the target's posterior range), and with `misfits`: best (the modelled data of
                        the first row of the least misfit among rows of positive weight), residual = yobs - best)],
            q, nmodels (weighted rows used), nexcluded (weighted rows left out: failed forward pass or NaN))
    ValueError for an empty selection or when the modelled data do not fit in device memory."""
    return _summarize(targets, models, vpvs, weights, misfits, mantle, q, nbins, device)


def best_rows(ci, w, misfits):
    """Per chain (ci sorted, as pool_selection returns it): the index of its first least-misfit row among the rows
    of positive weight -- np.argmin over what plot_bestdatafits reads of the chain."""
    pos = np.nonzero(np.asarray(w) > 0)[0]
    order = pos[np.lexsort((pos, np.asarray(misfits)[pos], np.asarray(ci)[pos]))]
    first = np.r_[True, ci[order][1:] != ci[order][:-1]]
    return order[first]


def pool_datafits(pool, selection='weighted', dev=0.05, exclude_outliers=True, q=DEFAULT_Q, nbins=100, device=None):
    """ChainPool.datafits: summarize() over the rows ChainPool.posterior uses, plus each chain's best fit."""
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    mis = pool.misfits[ci, ri, -1].astype(np.float64)
    pick = best_rows(ci, w, mis)
    res = _summarize(pool.targets, pool.models[ci, ri], pool.vpvs[ci, ri].astype(np.float64), w.astype(np.int32),
                     mis, pool.priors.get('mantle'), q, nbins, device, pick=pick)
    data = res.pop('_picked')
    res['bestfits'] = dict(chains=ci[pick] + pool.first, rows=ri[pick], data=data)
    res['chains'] = np.unique(ci) + pool.first
    return res


# ---- many sets of rows in one pass: the stations of a network ---------------------------------------------

class _FitsSets(_device.Handle):
    """One bh_datafits_sets handle over a device matrix whose rows come in contiguous sets."""

    def __init__(self, Y, ncols, weights, err, set_start, stream, chunk_bytes=None):
        self.ncols = ncols
        self.set_start = np.ascontiguousarray(set_start, dtype=np.int64)
        self.nsets = self.set_start.size - 1
        _device.Handle.__init__(
            self, 'datafits_sets', Y.data_ptr(), Y.shape[0], Y.stride(0), ncols, None if weights is None else
            weights.data_ptr(), None if err is None else err.data_ptr(), 0 if err is None else err.shape[1],
            self.set_start.ctypes.data, self.nsets, stream)
        if chunk_bytes is not None:
            _lib.check(self.lib.bh_datafits_sets_set_chunk_bytes(self.h, int(chunk_bytes)))

    def scan(self):
        """-> dict of arrays with one row per set, and 'status' (0: the set has statistics)."""
        S, N = self.nsets, self.ncols
        total, excl = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
        status = np.zeros(S, dtype=np.int32)
        vmin, vmax, mean = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N))
        _lib.check(self.lib.bh_datafits_sets_scan(self.h, total.ctypes.data, excl.ctypes.data, vmin.ctypes.data,
                                                  vmax.ctypes.data, mean.ctypes.data, status.ctypes.data))
        return dict(total=total, excluded=excl, vmin=vmin, vmax=vmax, mean=mean, status=status)

    def finish(self, ranks, edges, eset):
        """ranks [sets, nranks], edges [sets, targets, nbins + 1], eset [columns] -> (order statistics
        [sets, nranks, columns], histograms [sets, columns, nbins], std [sets, columns]); sets of non-zero status:
        NaN and 0."""
        S, N = self.nsets, self.ncols
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        eset = np.ascontiguousarray(eset, dtype=np.int32)
        nr = ranks.shape[1]
        ost = np.zeros((S, nr, N))
        hist = np.zeros((S, N, edges.shape[2] - 1), dtype=np.int64)
        std = np.zeros((S, N))
        _lib.check(self.lib.bh_datafits_sets_finish(
            self.h, ranks.ctypes.data if nr else None, nr, ost.ctypes.data if nr else None, edges.ctypes.data,
            edges.shape[2], edges.shape[1], eset.ctypes.data, hist.ctypes.data, std.ctypes.data))
        return ost, hist, std

    def status_text(self, status):
        return self.lib.bh_datafits_sets_status_text(int(status)).decode()


class _DeviceSets(object):
    """What summarize_sets does on the device: the forward pass of a run of rows into one matrix, the sets handle over
    it, and rows of the matrix back on the host.  (The CPU tier puts a numpy stand-in in its place.)"""

    def __init__(self, stations, mantle, device, rf_p, chunk_bytes=None):
        self.dev = _device.torch_device(device)
        self.joint, self.mantle, self.rf_p, self.chunk_bytes = stations[0], mantle, rf_p, chunk_bytes
        bl = self.joint.batch_layout(ell=True)
        desc, lay = bl['desc'], bl['layout']
        self.segs = [(desc[n].off, desc[n].off + desc[n].n) for n in range(self.joint.ntargets)]
        self.ncols = lay.ncols
        self.row_bytes = lay.row * 8 + bl['nflags'] * 4

    def max_rows(self):
        """rows whose matrix takes half of the free device memory (the other half: the handle's buffers and the
        layer temporaries of the forward pass)"""
        import torch
        return max(1, int(torch.cuda.mem_get_info(self.dev)[0] // (2 * self.row_bytes)))

    def forward(self, models, vpvs, set_id):
        _, Y, err, _ = forward_matrix(self.joint, models, vpvs, self.mantle, self.dev, self.rf_p, set_id)
        return Y, err

    def fits(self, Y, err, weights, set_start):
        import torch
        w = None if weights is None else _device.to_device(weights, torch.int32, self.dev)
        self._w = w                                    # alive as long as the handle
        return _FitsSets(Y, self.ncols, w, err, set_start, torch.cuda.current_stream(self.dev).cuda_stream,
                         self.chunk_bytes)

    def gather(self, Y, idx):
        import torch
        return Y[torch.as_tensor(np.asarray(idx, dtype=np.int64), device=self.dev)].cpu().numpy()

    def device(self):
        import torch
        return torch.cuda.device(self.dev)


def station_runs(set_start, max_rows):
    """Runs of whole sets whose rows fit `max_rows`, in order -> [(first set, one past the last)]: every set in
    exactly one run, a run closed before the set that would not fit any more; a set with more rows than max_rows is a
    run of its own (its matrix is refused, or not, where it is allocated)."""
    set_start = np.asarray(set_start, dtype=np.int64)
    S, runs, a = set_start.size - 1, [], 0
    if int(max_rows) < 1:
        raise ValueError("max_rows >= 1")
    for z in range(1, S + 1):
        if z == S or set_start[z + 1] - set_start[a] > max_rows:
            runs.append((a, z))
            a = z
    return runs


def set_ranks(q, totals):
    """order_ranks of every set of weight total totals[s] > 0 -> (per set its order_ranks tuple, or None for a total
    of 0; ranks [sets, n] for bh_datafits_sets_finish: every set's distinct ranks, a shorter list filled up with its
    last rank, zeros for a set without)."""
    rk = [order_ranks(q, int(W)) if W > 0 else None for W in totals]
    n = max([r[4].size for r in rk if r is not None] + [0])
    ranks = np.zeros((len(rk), n), dtype=np.int64)
    for z, r in enumerate(rk):
        if r is not None:
            ranks[z, :r[4].size] = r[4]
            ranks[z, r[4].size:] = r[4][-1]
    return rk, ranks


class SetFits(sel.SetList):
    """summarize_sets' list: entry s is summarize()'s dict of set s, or None for a set in `failed`
    ({set index: message})."""


def _summarize_sets(stations, models, set_start, vpvs, weights, misfits, mantle, q, nbins, device, rf_p, max_rows,
                    pick=None, chunk_bytes=None, backend=None):
    stations = list(stations)
    if not hasattr(models, 'shape') or not hasattr(models, 'dtype'):
        models = np.asarray(models)
    if models.ndim != 2:
        raise ValueError("models: [rows, 2*maxlayers]")
    R = models.shape[0]
    set_start, S = sel.check_set_start(set_start, R)
    if len(stations) != S:
        raise ValueError("one JointTarget per set")
    if int(nbins) < 1:
        raise ValueError("nbins >= 1")
    wh = None if weights is None else np.asarray(weights.cpu().numpy() if hasattr(weights, 'cpu') else weights)
    mf = None if misfits is None else np.asarray(misfits, dtype=np.float64)
    if wh is not None and wh.size != R or mf is not None and mf.size != R:
        raise ValueError("one weight and one misfit per row")
    vp = None if np.ndim(vpvs) == 0 else vpvs
    if vp is not None and len(vp) != R:
        raise ValueError("vpvs: one per row, or a scalar")
    if rf_p is not None and len(rf_p) != S:
        raise ValueError("rf_p: one row of ray parameters per station")
    be = backend if backend is not None else _DeviceSets(stations, mantle, device, rf_p, chunk_bytes)
    segs = be.segs
    results, failed = [None] * S, {}
    picked = None if pick is None else [None] * S
    pick = None if pick is None else np.asarray(pick, dtype=np.int64)
    for a, b in station_runs(set_start, be.max_rows() if max_rows is None else max_rows):
        lo, hi = int(set_start[a]), int(set_start[b])
        if hi == lo:
            for z in range(a, b):
                failed[z] = "empty selection: no models"
            continue
        start = set_start[a:b + 1] - lo
        ids = None if rf_p is None else np.repeat(np.arange(a, b, dtype=np.int32), np.diff(start))
        with be.device():
            Y, err = be.forward(models[lo:hi], vpvs if vp is None else vp[lo:hi], ids)
            with be.fits(Y, err, None if wh is None else wh[lo:hi], start) as f:
                s = f.scan()
                rk, ranks = set_ranks(q, np.where(s['status'] == 0, s['total'], 0))
                edges = np.zeros((b - a, len(segs), int(nbins) + 1))
                edges[:] = np.arange(int(nbins) + 1)         # (a set left out: anything ascending)
                eset = np.zeros(be.ncols, dtype=np.int32)
                for i in range(b - a):
                    if s['status'][i]:
                        failed[a + i] = f.status_text(s['status'][i])
                    else:
                        edges[i], eset = target_edges(s['vmin'][i], s['vmax'][i], segs, nbins)
                ost, hist, std = f.finish(ranks, edges, eset)
            live = [i for i in range(b - a) if not s['status'][i]]
            best = None
            if mf is not None and live:              # the first least-misfit row of positive weight within each set
                rows = []
                for i in live:
                    r0, r1 = lo + int(start[i]), lo + int(start[i + 1])
                    cand = np.arange(r0, r1) if wh is None else r0 + np.nonzero(wh[r0:r1] > 0)[0]
                    rows.append(int(cand[np.argmin(mf[cand])]) - lo)
                best = be.gather(Y, rows)
            if pick is not None:
                own = pick[(pick >= lo) & (pick < hi)]
                got = be.gather(Y, own - lo) if own.size else np.zeros((0, be.ncols))
                of = np.searchsorted(own, set_start[a:b + 1])
                for i in range(b - a):
                    picked[a + i] = [got[of[i]:of[i + 1], c0:c1] for c0, c1 in segs]
        for j, i in enumerate(live):
            sz = dict(total=int(s['total'][i]), excluded=int(s['excluded'][i]), vmin=s['vmin'][i], vmax=s['vmax'][i],
                      mean=s['mean'][i])
            results[a + i] = _result(stations[a + i], segs, sz, rk[i], ost[i][:rk[i][4].size], hist[i], std[i],
                                     edges[i], None if best is None else best[j], q)
            if pick is not None:
                results[a + i]['_picked'] = picked[a + i]
    return SetFits(results, failed)


def summarize_sets(stations, models, set_start, vpvs, weights=None, misfits=None, mantle=None, q=DEFAULT_Q, nbins=100,
                   device=None, rf_p=None, max_rows=None):
    """summarize() of every station of a network in one pass: station s owns the rows models[set_start[s]:
    set_start[s + 1]] (set_start [stations + 1], ascending from 0 to the number of rows; a station may have none),
    with their vpvs, weights and misfits.

    stations   sequence of JointTargets that share targets and axes (StationPool's rule): only obsdata.y differs --
               and, with rf_p, the ray parameter of the receiver functions
    rf_p       [stations, nrf] (stations.rf_slowness_table): every row is modelled at its own station's slowness
    max_rows   the stations are taken in runs of whole stations whose rows fit max_rows (default: what half of the free
               device memory holds), one forward pass and one bh_datafits_sets handle per run; no result depends on it

    -> SetFits: a list with summarize()'s dict per station, every field bit for bit what summarize returns for the
    station's rows alone, or None for a station without an included row of positive weight, whose message is in the
    list's `failed` {station index: message}.  A negative weight fails the call."""
    return _summarize_sets(stations, models, set_start, vpvs, weights, misfits, mantle, q, nbins, device, rf_p, max_rows)


class StationDatafits(sel.StationResult):
    """StationPool.datafits' result.

    stations   {station name: the dict pool.station(name).datafits(...) returns}, failed stations left out
    failed     {station name: message}
    names, refs   the pool's stations, the targets' refs
    mean, std, median, min, max, best, residual   per target (JointTarget order) [nstations, S], in the pool's station
               order; quantiles per target [nstations, len(q), S]; nmodels, nexcluded [nstations].  A failed station is
               a row of NaN (0 models)"""

    FIELDS = ('mean', 'std', 'median', 'min', 'max', 'best', 'residual')

    def __init__(self, names, results, failed, q):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {n: r for n, r in zip(names, results) if r is not None}
        self.q = np.asarray(q, dtype=np.float64)
        S = len(self.names)
        first = next((r for r in results if r is not None), None)
        self.refs = [] if first is None else [t['ref'] for t in first['targets']]
        size = [] if first is None else [t['mean'].size for t in first['targets']]
        for k in self.FIELDS:
            setattr(self, k, [np.full((S, n), np.nan) for n in size])
        self.quantiles = [np.full((S, self.q.size, n), np.nan) for n in size]
        self.nmodels, self.nexcluded = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
        for z, r in enumerate(results):
            if r is None:
                continue
            self.nmodels[z], self.nexcluded[z] = r['nmodels'], r['nexcluded']
            for t, d in enumerate(r['targets']):
                for k in self.FIELDS:
                    getattr(self, k)[t][z] = d[k]
                self.quantiles[t][z] = d['quantiles']


def stations_datafits(spool, selection='weighted', dev=0.05, exclude_outliers=True, q=DEFAULT_Q, nbins=100, device=None,
                      strict=True, max_rows=None, backend=None):
    """StationPool.datafits: summarize_sets() over every station's main-phase rows (see StationPool.datafits)."""
    pool, c = spool.pool, spool.chains_per_station
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    mis = pool.misfits[ci, ri, -1].astype(np.float64)
    pick = best_rows(ci, w, mis)
    rf_p = None
    if 'p' in spool.per_station:
        from .stations import rf_slowness_table
        rf_p = rf_slowness_table(spool.stations)
    res = _summarize_sets(spool.stations, pool.models[ci, ri], set_start, pool.vpvs[ci, ri].astype(np.float64),
                          w.astype(np.int32), mis, pool.priors.get('mantle'), q, nbins, device, rf_p, max_rows,
                          pick=pick, backend=backend)
    res.failed.update(failed)
    sel.raise_first_failed(res.failed, strict, "station", spool.names)
    for z, r in enumerate(res):
        if r is None:
            continue
        mine = pick[(pick >= set_start[z]) & (pick < set_start[z + 1])]
        r['bestfits'] = dict(chains=ci[mine] - z * c, rows=ri[mine], data=r.pop('_picked'))
        r['chains'] = sel.station_chains(ci, set_start, z, c)
    return StationDatafits(spool.names, res, res.failed, q)
