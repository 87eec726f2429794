"""Moho depth and crustal velocity of a block of sampled models, on the device (include/bayhunter_amd.h, bh_moho_*).

What the reference computes in PlotFromStorage.plot_moho_crustvel_tradeoff (src/Plotting.py:753-902): per posterior
model the Moho -- the shallowest interface inside a depth window below which Vs exceeds `mohovs` -- with the mean
crustal Vs above it, the Vs of the last crustal layer and the Vs jump (:766-798); then medians, a standard deviation,
four histograms and three joint histograms against the Moho depth with their modes (:813-865).

Every row carries an integer weight; the result equals the reference's on the matrix in which each row is repeated
`weight` times.  The per-row values are bit for bit numpy's on the row in its own dtype (csrc/moho_core.h); the
statistics of one set of rows go through the weighted column reduction of datafits (bh_datafits_* over the four
derived columns), the joint histograms and the per-station form through kernels of their own (csrc/moho.hip).
Edges are made here with numpy as np.histogram / np.histogram2d make them.
"""
import numpy as np

from . import _device, _lib, selection as sel      # (`selection` is a parameter of the entry points)
from .datafits import Fits

NAMES = ('moho', 'vs_crust', 'vs_last', 'vs_jump')          # the columns of the derived matrix
TRADEOFF = ('vs_last', 'vs_crust', 'vs_jump')               # x axes of the joint histograms, in the reference's order
_COL = {name: c for c, name in enumerate(NAMES)}


def _window(moho, mohovs, nbins):
    zlo, zhi = (float(v) for v in moho)
    mohovs = float(mohovs)
    if not zlo < zhi or np.isnan(mohovs):
        raise ValueError("moho: a depth window (zlo, zhi) with zlo < zhi; mohovs: a velocity")
    if int(nbins) < 1:
        raise ValueError("nbins >= 1")
    return zlo, zhi, mohovs, int(nbins)


def derive(rows, zlo, zhi, mohovs, stream):
    """bh_moho_rows over a device tensor of rows -> D [rows, 4] float64 on the same device, queued on `stream`."""
    import torch
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.shape[0] > 0
            and rows.dtype in (torch.float32, torch.float64) and rows.stride(1) == 1 and rows.stride(0) >= rows.shape[1]):
        raise ValueError("rows: a device tensor [rows, 2*maxlayers], float32 or float64, at least one row, "
                         "contiguous along a row")
    D = torch.empty((rows.shape[0], 4), dtype=torch.float64, device=rows.device)
    _lib.check(_lib.load().bh_moho_rows(rows.data_ptr(), int(rows.dtype.itemsize == 8), rows.shape[0], rows.stride(0),
                                        rows.shape[1], zlo, zhi, mohovs, D.data_ptr(), stream))
    return D


def outer_edges(vmin, vmax, nbins):
    """np.histogram's / np.histogram2d's edges for `bins=nbins`: linspace(min, max), +-0.5 when they are equal."""
    if vmin == vmax:
        vmin, vmax = vmin - 0.5, vmax + 0.5
    return np.linspace(vmin, vmax, nbins + 1)


def _no_moho(zlo, zhi, mohovs):
    return ValueError("no model has a Moho: no interface in the depth window (%g, %g) km with Vs > mohovs = %g km/s below it"
                      % (zlo, zhi, mohovs))


def summarize(models, weights=None, moho=(0., 100.), mohovs=4.2, nbins=50, device=None):
    """Moho statistics of `models` ([rows, 2*maxlayers], reference layout, float32 or float64; numpy or a torch
    tensor) with integer `weights` (>= 0, default 1 each), for the depth window moho = (zlo, zhi) and `mohovs`.

    -> dict(nmodels (weighted rows with a Moho), nexcluded (weighted rows without one),
            moho, vs_crust, vs_last, vs_jump = dict(median, mean, std, min, max, hist = (counts, edges)) each,
            tradeoff = {vs_last, vs_crust, vs_jump: dict(counts [nbins, nbins] (x index first, as np.histogram2d),
                        xedges, yedges, mode = (x, y): the cell centres of the first maximum in C order)})
    ValueError when no row has a Moho."""
    import torch
    zlo, zhi, mohovs, nbins = _window(moho, mohovs, nbins)
    dev, rows, w, _ = _device.device_rows(models, weights, per_row="one weight per row", device=device)
    if rows.shape[0] == 0:
        raise ValueError("empty selection: no models")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        D = derive(rows, zlo, zhi, mohovs, stream)
        with Fits(D, 4, w, None, stream) as f:
            try:
                s = f.scan()
            except _lib.BayHunterAmdError as e:
                if 'empty selection' in str(e):          # scan_fault()'s words (csrc/stats_host.h)
                    raise _no_moho(zlo, zhi, mohovs)
                raise
            W = s['total']
            edges = np.stack([outer_edges(s['vmin'][c], s['vmax'][c], nbins) for c in range(4)])
            ost, hist, std = f.finish(np.array([(W - 1) // 2, W // 2], dtype=np.int64), edges, np.arange(4, dtype=np.int32))
        xedges = np.ascontiguousarray(edges[[_COL[n] for n in TRADEOFF]])
        h2 = np.zeros((3, nbins, nbins), dtype=np.int64)
        _lib.check(lib.bh_moho_hist2d(D.data_ptr(), D.shape[0], None if w is None else w.data_ptr(), xedges.ctypes.data,
                                      edges[0].ctypes.data, nbins + 1, h2.ctypes.data, stream))
    median = (ost[0] + ost[1]) / 2.
    res = dict(nmodels=W, nexcluded=s['excluded'], tradeoff={})
    for c, name in enumerate(NAMES):
        res[name] = dict(median=median[c], mean=s['mean'][c], std=std[c], min=s['vmin'][c], max=s['vmax'][c],
                         hist=(hist[c], edges[c]))
    yc = (edges[0][:-1] + edges[0][1:]) / 2.
    for i, name in enumerate(TRADEOFF):
        xi, yi = np.unravel_index(h2[i].argmax(), h2[i].shape)
        xc = (xedges[i][:-1] + xedges[i][1:]) / 2.
        res['tradeoff'][name] = dict(counts=h2[i], xedges=xedges[i], yedges=edges[0], mode=(xc[xi], yc[yi]))
    return res


def _tradeoff_sets(D, w, set_start, vmin, vmax, nbins, stream):
    """summarize()'s `tradeoff` of every set over D = derive()'s matrix: the x columns of TRADEOFF against the Moho
    depth over each set's own outer_edges (vmin, vmax [sets, 4]: NaN for a set without a Moho), one bh_hist2d_sets
    launch -> {name: dict(counts [sets, nbins, nbins], xedges, yedges [sets, nbins + 1], mode [sets, 2])}."""
    S = set_start.size - 1
    has = ~np.isnan(vmin[:, 0])
    edges = np.zeros((S, 4, nbins + 1))
    edges[:] = np.arange(nbins + 1)                     # (a set without a Moho adds nothing: anything ascending)
    for z in np.nonzero(has)[0]:
        edges[z] = [outer_edges(vmin[z, c], vmax[z, c], nbins) for c in range(4)]
    pairs = np.array([(_COL[n], 0) for n in TRADEOFF], dtype=np.int32)
    h2 = np.zeros((S, 3, nbins, nbins), dtype=np.int64)
    _lib.check(_lib.load().bh_hist2d_sets(D.data_ptr(), D.shape[0], D.stride(0), 4, None if w is None else w.data_ptr(),
                                          set_start.ctypes.data, S, pairs.ctypes.data, 3, edges.ctypes.data, nbins + 1,
                                          h2.ctypes.data, stream))
    edges[~has] = np.nan
    yc = (edges[:, 0, :-1] + edges[:, 0, 1:]) / 2.
    out = {}
    for i, name in enumerate(TRADEOFF):
        xe = edges[:, _COL[name]]
        xc = (xe[:, :-1] + xe[:, 1:]) / 2.
        xi, yi = np.unravel_index(h2[:, i].reshape(S, -1).argmax(axis=1), (nbins, nbins))
        out[name] = dict(counts=h2[:, i].copy(), xedges=xe.copy(), yedges=edges[:, 0].copy(),
                         mode=np.stack((xc[np.arange(S), xi], yc[np.arange(S), yi]), axis=1))
    return out


def summarize_sets(models, set_start, weights=None, moho=(0., 100.), mohovs=4.2, nbins=50, device=None, tradeoff=False):
    """summarize()'s numbers for every set of rows in one pass: set s is models[set_start[s]:set_start[s + 1]]
    (set_start [sets + 1], ascending from 0 to the number of rows; a set may be empty).  One derivation launch and one
    launch for the statistics of all sets.

    -> dict(nmodels, nexcluded [sets] (weighted rows with / without a Moho), fraction [sets] (nmodels over both; NaN for
            a set without weight), moho, vs_crust, vs_last, vs_jump = dict(median, mean, std, min, max [sets]) each,
            hist [sets, nbins] of the Moho depth over the shared `edges` = linspace(zlo, zhi, nbins + 1));
            with tradeoff=True also tradeoff = {vs_last, vs_crust, vs_jump: dict(counts [sets, nbins, nbins], xedges,
            yedges [sets, nbins + 1], mode [sets, 2])}: summarize()'s three joint histograms of every set over the set's
            own edges, from one more launch (bh_hist2d_sets, nbins <= 64).
    A set without a row that has a Moho is no error: nmodels 0, its statistics NaN, its histogram empty (the edges and
    modes of its trade-off NaN).  A negative weight fails the call."""
    import torch
    zlo, zhi, mohovs, nbins = _window(moho, mohovs, nbins)
    if tradeoff and nbins > _lib.PAIRS_MAX_EDGES - 1:
        raise ValueError("tradeoff: nbins <= %d" % (_lib.PAIRS_MAX_EDGES - 1))
    dev, rows, w, _ = _device.device_rows(models, weights, per_row="one weight per row", device=device)
    set_start, S = sel.check_set_start(set_start, rows.shape[0])
    edges = np.linspace(zlo, zhi, nbins + 1)
    cnt, nex = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    st = {k: np.full((S, 4), np.nan) for k in ('min', 'max', 'mean', 'std', 'lo', 'hi')}
    hist = np.zeros((S, nbins), dtype=np.int64)
    trade = None
    if tradeoff and not rows.shape[0]:
        nan = lambda *shape: np.full(shape, np.nan)
        trade = {n: dict(counts=np.zeros((S, nbins, nbins), dtype=np.int64), xedges=nan(S, nbins + 1),
                         yedges=nan(S, nbins + 1), mode=nan(S, 2)) for n in TRADEOFF}
    if rows.shape[0]:
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            D = derive(rows, zlo, zhi, mohovs, stream)
            _lib.check(_lib.load().bh_moho_sets(
                D.data_ptr(), D.shape[0], None if w is None else w.data_ptr(), set_start.ctypes.data, S,
                edges.ctypes.data, nbins + 1, cnt.ctypes.data, nex.ctypes.data, st['min'].ctypes.data,
                st['max'].ctypes.data, st['mean'].ctypes.data, st['std'].ctypes.data, st['lo'].ctypes.data,
                st['hi'].ctypes.data, hist.ctypes.data, stream))
            if tradeoff:
                trade = _tradeoff_sets(D, w, set_start, st['min'], st['max'], nbins, stream)
    median = (st['lo'] + st['hi']) / 2.
    with np.errstate(invalid='ignore', divide='ignore'):
        fraction = np.where(cnt + nex > 0, cnt / (cnt + nex).astype(np.float64), np.nan)
    res = dict(nmodels=cnt, nexcluded=nex, fraction=fraction, hist=hist, edges=edges)
    for c, name in enumerate(NAMES):
        res[name] = dict(median=median[:, c].copy(), mean=st['mean'][:, c].copy(), std=st['std'][:, c].copy(),
                         min=st['min'][:, c].copy(), max=st['max'][:, c].copy())
    if tradeoff:
        res['tradeoff'] = trade
    return res


def _widened(models, device):
    """A pool's float32 rows on the device as float64: save() writes them as float64 (the reference fills float64
    matrices, src/Models.py:228-274), so that is the dtype in which PlotFromStorage derives the Moho from them."""
    import torch
    return _device.to_device(models, torch.float32 if models.dtype == np.float32 else torch.float64,
                             _device.torch_device(device)).to(torch.float64)


def pool_moho(pool, moho=None, mohovs=4.2, selection='weighted', dev=0.05, exclude_outliers=True, nbins=50, device=None):
    """ChainPool.moho: summarize() over the rows ChainPool.posterior uses, plus 'chains' (global indices used)."""
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    res = summarize(_widened(pool.models[ci, ri], device), w.astype(np.int32), pool.priors['z'] if moho is None else moho,
                    mohovs, nbins, device)
    res['chains'] = np.unique(ci) + pool.first
    return res


class StationMoho(sel.StationResult):
    """StationPool.moho's result, every array in the pool's station order.

    names      the stations
    moho, vs_crust, vs_last, vs_jump   dict(median, mean, std, min, max [nstations]) each; NaN for a station without a
               model that has a Moho (a hole of the Moho map) and for a failed one
    nmodels, nexcluded [nstations]     weighted rows with / without a Moho
    fraction [nstations]               nmodels / (nmodels + nexcluded)
    hist [nstations, nbins], edges     the Moho depth over edges all stations share: linspace(zlo, zhi, nbins + 1)
    tradeoff   with tradeoff=True only: {vs_last, vs_crust, vs_jump: dict(counts [nstations, nbins, nbins], xedges, yedges
               [nstations, nbins + 1], mode [nstations, 2])}, every station over its own edges
    failed     {station name: message}, as StationPool.posterior reports it (such a station has no rows)"""

    def __init__(self, names, res, failed):
        sel.StationResult.__init__(self, names, failed)
        for k, v in res.items():
            setattr(self, k, v)


def stations_moho(spool, moho=None, mohovs=4.2, selection='weighted', dev=0.05, exclude_outliers=True, nbins=50,
                  device=None, tradeoff=False):
    """StationPool.moho: summarize_sets() over every station's main-phase rows."""
    pool, c = spool.pool, spool.chains_per_station
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    res = summarize_sets(_widened(pool.models[ci, ri], device), set_start, w.astype(np.int32),
                         pool.priors['z'] if moho is None else moho, mohovs, nbins, device, tradeoff)
    return StationMoho(spool.names, res, failed)
