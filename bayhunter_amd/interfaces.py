"""Discontinuity statistics of a block of sampled models, on the device (include/bayhunter_amd.h, bh_interfaces_sets).

Where a transdimensional posterior puts its interfaces and which way Vs steps across them: per depth bin the
probability that a model has an interface there, a negative one (the top of a low-velocity zone, a mid-lithospheric
discontinuity, the lithosphere-asthenosphere boundary) or a positive one (the base of the sediments, a mid-crustal
step, the Moho), the joint histogram of interface depth and Vs jump, and the mean and spread of the jump.

A row with n nuclei has the interfaces k = 0 .. n-2 at the depths of posterior.stepmodel (z_disc midpoints, the
sequential float64 cumsum) with the jumps J_k = float64(vs[k+1]) - float64(vs[k]).  Every row carries an integer
weight; the result equals that of the matrix in which each row is repeated `weight` times.  Bins follow numpy's
rule (the last bin closed); an interface outside the depth edges adds nothing, a jump outside the jump edges is left
out of `hist` only.  The walk and the order of the two float sums: csrc/interfaces_core.h; the kernels:
csrc/interfaces.hip.
"""
import numpy as np

from . import _device, _lib, selection as sel      # (`selection` is a parameter of the entry points)
from .posterior import hist_grids

COUNTS = ('count', 'models', 'neg', 'pos', 'models_neg', 'models_pos')     # int64 [depth bins] each
SECTION = ('p_interface', 'p_neg', 'p_pos', 'jump_mean', 'count')          # what StationPool.interfaces stacks
_EMPTY = "empty selection (no row with a positive weight)"


def default_jump_edges():
    return np.linspace(-2, 2, 41)


def _edges(dep_edges, jump_edges):
    """The two edge arrays as contiguous float64, checked as the library checks them."""
    de = hist_grids(None)[1] if dep_edges is None else dep_edges
    je = default_jump_edges() if jump_edges is None else jump_edges
    out = []
    for name, e, most in (('dep_edges', de, _lib.INTERFACES_MAX_DEPTH_BINS), ('jump_edges', je, _lib.INTERFACES_MAX_JUMP_BINS)):
        e = np.ascontiguousarray(e, dtype=np.float64)
        if e.ndim != 1 or e.size < 2 or e.size > most + 1:
            raise ValueError("%s: 2 to %d edges" % (name, most + 1))
        if not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0):
            raise ValueError("%s: finite and ascending" % name)
        out.append(e)
    return out


def _rows(models, weights, device):
    """device_rows, after what can be refused on the host: the width, and a negative weight in host weights."""
    shape = getattr(models, 'shape', None) or np.asarray(models).shape
    if len(shape) != 2:
        raise ValueError("models: [rows, 2*maxlayers]")
    if shape[1] < 2 or shape[1] > 2 * _lib.MAX_LAYERS + 2:
        raise ValueError("models: 2 to %d columns" % (2 * _lib.MAX_LAYERS + 2))
    if weights is not None and not hasattr(weights, 'is_cuda') and np.any(np.asarray(weights) < 0):
        raise ValueError("negative weight")
    return _device.device_rows(models, weights, per_row="one weight per row", device=device)


def _reduce(dev, rows, w, set_start, dedges, jedges):
    """One bh_interfaces_sets call -> dict of arrays with one row per set."""
    import torch
    S, nbd, nbj = set_start.size - 1, dedges.size - 1, jedges.size - 1
    res = dict(total=np.zeros(S, dtype=np.int64), hist=np.zeros((S, nbd, nbj), dtype=np.int64),
               jsum=np.full((S, nbd), np.nan), jsq=np.full((S, nbd), np.nan))
    for k in COUNTS:
        res[k] = np.zeros((S, nbd), dtype=np.int64)
    if rows.shape[0]:
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(_lib.load().bh_interfaces_sets(
                rows.data_ptr(), int(rows.dtype.itemsize == 8), rows.shape[0], rows.stride(0), rows.shape[1],
                None if w is None else w.data_ptr(), set_start.ctypes.data, S, dedges.ctypes.data, dedges.size,
                jedges.ctypes.data, jedges.size, res['total'].ctypes.data, res['count'].ctypes.data,
                res['models'].ctypes.data, res['neg'].ctypes.data, res['pos'].ctypes.data,
                res['models_neg'].ctypes.data, res['models_pos'].ctypes.data, res['hist'].ctypes.data,
                res['jsum'].ctypes.data, res['jsq'].ctypes.data, stream))
    return res


def _result(res, z, dedges, jedges):
    """summarize()'s dict of set z, or None for a set without weight."""
    total = int(res['total'][z])
    if total == 0:
        return None
    out = {k: res[k][z].copy() for k in COUNTS + ('hist', 'jsum', 'jsq')}
    out['total'] = total
    cnt = out['count']
    with np.errstate(invalid='ignore', divide='ignore'):
        out['jump_mean'] = np.where(cnt > 0, out['jsum'] / cnt, np.nan)
        out['jump_std'] = np.where(cnt > 0, np.sqrt(out['jsq'] / cnt), np.nan)
    out['p_interface'] = out['models'] / float(total)
    out['p_neg'] = out['models_neg'] / float(total)
    out['p_pos'] = out['models_pos'] / float(total)
    out['dep_edges'], out['jump_edges'] = dedges, jedges
    return out


def summarize(models, weights=None, dep_edges=None, jump_edges=None, device=None):
    """Discontinuity statistics of `models` ([rows, 2*maxlayers], reference layout, float32 or float64; numpy or a
    torch tensor) with integer `weights` (>= 0, default 1 each).

    dep_edges    depth bin edges (default: the posterior's own interface edges, posterior.hist_grids(None)[1])
    jump_edges   Vs-jump bin edges (default linspace(-2, 2, 41) km/s)

    -> dict(total (the weighted number of models, those without an interface included),
            count, neg, pos [depth bins]  the weight of the interfaces in the bin; with a jump < 0; with a jump > 0,
            models, models_neg, models_pos [depth bins]  the same, a model counted once per bin,
            p_interface, p_neg, p_pos = models / total, ...: the probability of an interface per depth bin,
            hist [depth bins, jump bins], jsum, jsq, jump_mean, jump_std [depth bins] (NaN where count is 0),
            dep_edges, jump_edges)
    With the default dep_edges, `count` is posterior.summarize()['interfaces'][0].  ValueError for an empty selection."""
    dedges, jedges = _edges(dep_edges, jump_edges)
    dev, rows, w, _ = _rows(models, weights, device)
    if rows.shape[0] == 0:
        raise ValueError("empty selection: no models")
    res = _reduce(dev, rows, w, np.array([0, rows.shape[0]], dtype=np.int64), dedges, jedges)
    out = _result(res, 0, dedges, jedges)
    if out is None:
        raise ValueError(_EMPTY)
    return out


class SetResults(sel.SetList):
    """summarize_sets' list: entry s is summarize()'s dict of set s, or None for a set in `failed`."""

    def __init__(self, results, failed, dedges):
        sel.SetList.__init__(self, results, failed)
        self.dep_edges = dedges

    def section(self):
        """p_interface / p_neg / p_pos / jump_mean / count stacked [sets, depth bins] (float64), a failed set a row
        of NaN."""
        out = {k: np.full((len(self), self.dep_edges.size - 1), np.nan) for k in SECTION}
        for z, res in enumerate(self):
            if res is not None:
                for k in SECTION:
                    out[k][z] = res[k]
        return out


def summarize_sets(models, set_start, weights=None, dep_edges=None, jump_edges=None, device=None, strict=True):
    """summarize() of every set of rows in one pass: set s is models[set_start[s]:set_start[s + 1]] (set_start
    [sets + 1], ascending from 0 to the number of rows; a set may be empty).  The edges are shared by all sets.

    -> SetResults: a list with summarize()'s dict per set, every field bit for bit what summarize returns for the
    set's rows alone.  A set without a row of positive weight raises a ValueError naming the first such set -- or,
    with strict=False, has the entry None and its message in the list's `failed`.  A negative weight fails the call."""
    dedges, jedges = _edges(dep_edges, jump_edges)
    dev, rows, w, _ = _rows(models, weights, device)
    set_start, S = sel.check_set_start(set_start, rows.shape[0])
    res = _reduce(dev, rows, w, set_start, dedges, jedges)
    results = [_result(res, z, dedges, jedges) for z in range(S)]
    failed = {z: _EMPTY for z in range(S) if results[z] is None}
    sel.raise_first_failed(failed, strict, "set")
    return SetResults(results, failed, dedges)


def pool_interfaces(pool, dep_edges=None, jump_edges=None, selection='weighted', dev=0.05, exclude_outliers=True,
                    device=None):
    """ChainPool.interfaces: summarize() over the rows ChainPool.posterior uses, plus 'chains' (global indices used)."""
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    res = summarize(pool.models[ci, ri], w.astype(np.int32), dep_edges, jump_edges, device)
    res['chains'] = np.unique(ci) + pool.first
    return res


class StationInterfaces(sel.StationResult):
    """StationPool.interfaces' result.

    stations   {station name: the dict pool.station(name).interfaces(...) returns}, stations without a model left out
    failed     {station name: message}
    dep_edges, jump_edges   the edges all stations share
    p_interface, p_neg, p_pos, jump_mean, count [nstations, depth bins]   the discontinuity section along the pool's
               station order (float64); a station without a model is a row of NaN"""

    def __init__(self, names, results, failed, jedges):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {n: r for n, r in zip(names, results) if r is not None}
        self.dep_edges, self.jump_edges = results.dep_edges, jedges
        for k, v in results.section().items():
            setattr(self, k, v)


def stations_interfaces(spool, dep_edges=None, jump_edges=None, selection='weighted', dev=0.05, exclude_outliers=True,
                        device=None):
    """StationPool.interfaces: summarize_sets() over every station's main-phase rows."""
    pool, c = spool.pool, spool.chains_per_station
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    res = summarize_sets(pool.models[ci, ri], set_start, w.astype(np.int32), dep_edges, jump_edges, device, strict=False)
    res.failed.update(failed)
    for z, r in enumerate(res):
        if r is not None:
            r['chains'] = sel.station_chains(ci, set_start, z, c)
    return StationInterfaces(spool.names, res, res.failed, _edges(dep_edges, jump_edges)[1])
