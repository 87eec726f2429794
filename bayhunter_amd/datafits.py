"""Posterior statistics of the modelled data, on the device (include/bayhunter_amd.h, bh_datafits_*).

The reference looks at the data fit of an inversion one model per chain (PlotFromStorage.plot_bestdatafits,
src/Plotting.py:1054-1111; plot_rfcorr, :1114-1150): the least-misfit saved model of each chain through
target.moddata.plugin.run_model.  Here every sampled row goes through the batched forward pass
(models.layers_from_voronoi -> ForwardEngine.run, into one device matrix) and the library reduces every
column of that matrix over the weighted rows: mean, std, min, max, exact percentiles and a histogram per
sample (the "data fan"), as on the matrix in which every row is repeated `weight` times.

Rows whose forward pass failed (a dispersion search that found no root) or whose modelled data hold a NaN
are left out and counted (`nexcluded`, in weighted rows).
"""
import ctypes as C

import numpy as np

from . import _lib
from .posterior import _Handle, _to_device, _torch_device, pool_rows

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


class _Fits(_Handle):
    """One bh_datafits handle over a device matrix."""

    def __init__(self, Y, ncols, weights, err, stream):
        self.ncols = ncols
        _Handle.__init__(
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


def forward_matrix(targets, models, vpvs, mantle=None, device=None):
    """The modelled data of every row on the device -> (engine, Y [rows, engine.row] fp64, err [rows, nflags],
    batch layout).  Layers: layers_from_voronoi (Model.get_vp_vs_h, rho = 0.77 + 0.32 vp) in chunks."""
    import torch
    from .engine import ForwardEngine
    from .models import layers_from_voronoi
    dev = _torch_device(device)
    bl = targets.batch_layout()
    lay = bl['layout']
    with torch.cuda.device(dev):
        eng = ForwardEngine(swd=lay.swd, rf=lay.rf, device=dev)
        rows = _to_device(models, torch.float64, dev)
        vpvs = _to_device(np.broadcast_to(np.asarray(vpvs, dtype=np.float64), (rows.shape[0],))
                          if not isinstance(vpvs, torch.Tensor) else vpvs, torch.float64, dev)
        R = rows.shape[0]
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
            eng.run(dm, out=Y[lo:hi], err=err[lo:hi])
    return eng, Y, err, bl


def _summarize(targets, models, vpvs, weights, misfits, mantle, q, nbins, device, pick=None):
    import torch
    dev = _torch_device(device)
    if not isinstance(models, torch.Tensor):
        models = np.asarray(models)
    if models.ndim != 2 or models.shape[0] == 0:
        raise ValueError("models: [rows, 2*maxlayers], at least one row")
    R = models.shape[0]
    if int(nbins) < 1:
        raise ValueError("nbins >= 1")
    w = None if weights is None else _to_device(weights, torch.int32, dev)
    if w is not None and w.numel() != R or misfits is not None and np.asarray(misfits).size != R:
        raise ValueError("one weight and one misfit per row")
    eng, Y, err, bl = forward_matrix(targets, models, vpvs, mantle, dev)
    desc = bl['desc']
    segs = [(desc[n].off, desc[n].off + desc[n].n) for n in range(targets.ntargets)]
    ncols = eng.ncols
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        with _Fits(Y, ncols, w, err, stream) as f:
            s = f.scan()
            W = s['total']
            virt, lo, hi = percentile_ranks(q, W)
            med = np.array([(W - 1) // 2, W // 2], dtype=np.int64)
            ranks = np.unique(np.concatenate((lo, hi, med)))
            if ranks.size > _lib.MAX_DATAFITS_RANKS:
                raise ValueError("too many percentiles: at most %d distinct order statistics" % _lib.MAX_DATAFITS_RANKS)
            eset = np.zeros(ncols, dtype=np.int32)
            edges = np.zeros((len(segs), int(nbins) + 1))
            for t, (a, b) in enumerate(segs):
                tmin, tmax = s['vmin'][a:b].min(), s['vmax'][a:b].max()
                if tmin == tmax:
                    tmin, tmax = tmin - 0.5, tmax + 0.5
                edges[t] = np.linspace(tmin, tmax, int(nbins) + 1)
                eset[a:b] = t
            ost, hist, std = f.finish(ranks, edges, eset)
        picked = None if pick is None else Y[torch.as_tensor(np.asarray(pick, dtype=np.int64), device=dev)].cpu().numpy()
        best = None
        if misfits is not None:
            mf = np.asarray(misfits, dtype=np.float64)
            wh = np.ones(R, dtype=bool) if weights is None else np.asarray(
                weights.cpu().numpy() if isinstance(weights, torch.Tensor) else weights) > 0
            cand = np.nonzero(wh)[0]
            best = Y[int(cand[np.argmin(mf[cand])])].cpu().numpy()
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
    res = dict(targets=out, q=np.asarray(q, dtype=np.float64), nmodels=W, nexcluded=s['excluded'])
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
    ci, ri, w = pool_rows(pool, selection, dev, exclude_outliers)
    mis = pool.misfits[ci, ri, -1].astype(np.float64)
    pick = best_rows(ci, w, mis)
    res = _summarize(pool.targets, pool.models[ci, ri], pool.vpvs[ci, ri].astype(np.float64), w.astype(np.int32),
                     mis, pool.priors.get('mantle'), q, nbins, device, pick=pick)
    data = res.pop('_picked')
    res['bestfits'] = dict(chains=ci[pick] + pool.first, rows=ri[pick], data=data)
    res['chains'] = np.unique(ci) + pool.first
    return res
