"""Posterior cross-covariance of the Vs(z) profile and the modelled data, on the device: which depth range a datum -- one
period of a dispersion curve, one H/V value, one sample of a receiver function -- moves with across the ensemble.

People draw sensitivity kernels around a single model to see what a datum constrains.  The posterior holds the answer
for the whole ensemble, non-linearity and trade-offs included: corr[k, j] near +-1 says datum j and Vs at depth k move
together over the sampled models, near 0 that the datum says nothing about that depth here; with 'vpvs' as an extra row
it shows which data pin Vp/Vs.  The reference has no counterpart.

Every row carries an integer weight; the result equals the cross block of np.cov(np.hstack((X, Y)).T, bias=True) on the
matrices in which each row's Vs on the depth grid (and its extra values) and its modelled data are repeated `weight`
times, without building them.  The modelled data come from one forward pass (datafits.forward_matrix); the centres are
the two segmented scans' means (posterior.Sets.scan for Vs, bh_datafits_sets_scan for the data, which also says which
rows count: a row whose forward pass failed or whose modelled data hold a NaN is left out and counted in `nexcluded`,
as datafits does); the one new device part is bh_datacov_sets (csrc/datacov.hip): per set C = sum w dx dy^T with the
first and the diagonal second moments of both sides, on the FP64 matrix cores.  What is left is from_moments() below,
which needs no device.
"""
import numpy as np

from . import _device, _lib, datafits as df, posterior as post, selection as sel
from .covariance import column_names


# ---- the rules, without a device ------------------------------------------------------------------------

def from_moments(C, r1x, r1y, qx, qy, W, constant_x=None, constant_y=None):
    """Cross-covariance, correlation and the two standard deviations from the centred moments of one set: C [K, S] =
    sum w dx dy^T, r1x [K] = sum w dx, r1y [S] = sum w dy, qx [K] = sum w dx^2, qy [S] = sum w dy^2, W = sum w, with
    dx = x - cx and dy = y - cy for ANY centres:

        cov = (C - r1x r1y^T / W) / W      (population; r1 takes out what the centres are off the means)
        var_x = (qx - r1x^2 / W) / W,  var_y = (qy - r1y^2 / W) / W,  corr = cov / (std_x std_y^T)

    constant_x [K], constant_y [S] mark columns known to hold one value (their min equals their max): their variance is
    exactly 0, whatever the rounding of the centre left in q.  A model column of variance 0 has std 0, a row of zeros in
    cov and a row of NaN in corr; a data column of variance 0 the same in its column: the rule of
    covariance.from_moments.  -> (cov, corr, std_x, std_y)."""
    C, r1x, r1y = (np.asarray(a, dtype=np.float64) for a in (C, r1x, r1y))
    qx, qy = np.asarray(qx, dtype=np.float64), np.asarray(qy, dtype=np.float64)
    K, S = r1x.size, r1y.size
    if C.shape != (K, S) or qx.shape != (K,) or qy.shape != (S,) or r1x.ndim != 1 or r1y.ndim != 1 or not W > 0:
        raise ValueError("from_moments: C [K, S], r1x, qx [K], r1y, qy [S] and a weight total above 0")
    W = float(W)
    cov = (C - np.outer(r1x, r1y) / W) / W
    var_x, var_y = (qx - r1x * r1x / W) / W, (qy - r1y * r1y / W) / W
    flat_x, flat_y = var_x <= 0, var_y <= 0
    if constant_x is not None:
        flat_x |= np.asarray(constant_x, dtype=bool)
    if constant_y is not None:
        flat_y |= np.asarray(constant_y, dtype=bool)
    cov[flat_x, :] = 0.
    cov[:, flat_y] = 0.
    var_x[flat_x] = 0.
    var_y[flat_y] = 0.
    std_x, std_y = np.sqrt(var_x), np.sqrt(var_y)
    with np.errstate(invalid='ignore', divide='ignore'):
        corr = cov / np.outer(std_x, std_y)
    corr[flat_x, :] = np.nan
    corr[:, flat_y] = np.nan
    return cov, corr, std_x, std_y


# ---- on the device ------------------------------------------------------------------------------------------

def datacov_sets(rows, weights, extra, Y, ncols, err, set_start, dep, cx, cy, stream, col0=0):
    """bh_datacov_sets over device rows (weights: int32 device tensor or None; extra: float64 device matrix or None), the
    float64 device matrix Y of their modelled data -- the data columns are col0 .. col0 + ncols - 1 -- and its int32 err
    flags (or None) -> dict(C [sets, K, S], r1x, qx [sets, K], r1y, qy [sets, S], total, excluded [sets])."""
    set_start = np.ascontiguousarray(set_start, dtype=np.int64)
    dep = np.ascontiguousarray(dep, dtype=np.float64)
    Z, nextra, S = set_start.size - 1, 0 if extra is None else extra.shape[1], int(ncols)
    K = dep.size + nextra
    cx, cy = np.ascontiguousarray(cx, dtype=np.float64), np.ascontiguousarray(cy, dtype=np.float64)
    if cx.shape != (Z, K) or cy.shape != (Z, S):
        raise ValueError("cx: [sets, depths + extra columns], cy: [sets, data columns]")
    out = dict(C=np.zeros((Z, K, S)), r1x=np.zeros((Z, K)), r1y=np.zeros((Z, S)), qx=np.zeros((Z, K)), qy=np.zeros((Z, S)),
               total=np.zeros(Z, dtype=np.int64), excluded=np.zeros(Z, dtype=np.int64))
    _lib.check(_lib.load().bh_datacov_sets(
        rows.data_ptr(), int(rows.dtype.itemsize == 8), rows.shape[0], rows.stride(0), rows.shape[1],
        None if weights is None else weights.data_ptr(), None if extra is None else extra.data_ptr(),
        0 if extra is None else extra.stride(0), nextra, Y.data_ptr(), Y.stride(0), int(col0), S,
        None if err is None else err.data_ptr(), 0 if err is None else err.stride(0), 0 if err is None else err.shape[1],
        set_start.ctypes.data, Z, dep.ctypes.data, dep.size, cx.ctypes.data, cy.ctypes.data, out['C'].ctypes.data,
        out['r1x'].ctypes.data, out['r1y'].ctypes.data, out['qx'].ctypes.data, out['qy'].ctypes.data,
        out['total'].ctypes.data, out['excluded'].ctypes.data, stream))
    return out


class ColumnScan(_device.Handle):
    """The scan of one bh_datafits_sets handle over a device matrix whose rows come in contiguous sets: per set the weight
    total of the rows it keeps, the weight it leaves out, and min, max and mean of every column."""

    def __init__(self, Y, ncols, weights, err, set_start, stream):
        self.ncols = int(ncols)
        self.set_start = np.ascontiguousarray(set_start, dtype=np.int64)
        self.nsets = self.set_start.size - 1
        _device.Handle.__init__(
            self, 'datafits_sets', Y.data_ptr(), Y.shape[0], Y.stride(0), self.ncols, None if weights is None else
            weights.data_ptr(), None if err is None else err.data_ptr(), 0 if err is None else err.shape[1],
            self.set_start.ctypes.data, self.nsets, stream)

    def scan(self):
        Z, N = self.nsets, self.ncols
        total, excl, status = np.zeros(Z, dtype=np.int64), np.zeros(Z, dtype=np.int64), np.zeros(Z, dtype=np.int32)
        vmin, vmax, mean = np.zeros((Z, N)), np.zeros((Z, N)), np.zeros((Z, N))
        _lib.check(self.lib.bh_datafits_sets_scan(self.h, total.ctypes.data, excl.ctypes.data, vmin.ctypes.data,
                                                  vmax.ctypes.data, mean.ctypes.data, status.ctypes.data))
        return dict(total=total, excluded=excl, vmin=vmin, vmax=vmax, mean=mean, status=status)

    def status_text(self, status):
        return self.lib.bh_datafits_sets_status_text(int(status)).decode()


def check_columns(dep_int, extra, extra_names, nrows):
    """The model side's arguments -> (dep_int, extra_names, nextra)."""
    dep_int = post.default_dep_int() if dep_int is None else np.ascontiguousarray(dep_int, dtype=np.float64)
    if dep_int.ndim != 1 or dep_int.size < 1 or np.any(np.isnan(dep_int)) or np.any(np.diff(dep_int) <= 0):
        raise ValueError("dep_int: one depth at least, ascending")
    extra_names = [str(n) for n in extra_names]
    nextra = 0 if extra is None else (extra.shape[1] if len(extra.shape) == 2 else -1)
    if nextra < 0 or (extra is not None and extra.shape[0] != nrows):
        raise ValueError("extra: [rows, columns], one row per model")
    if len(extra_names) != nextra or len(set(extra_names)) != nextra:
        raise ValueError("extra_names: one distinct name per column of extra")
    if dep_int.size + nextra > _lib.DEPTHCOV_MAX_K:
        raise ValueError("at most %d depths and extra columns together" % _lib.DEPTHCOV_MAX_K)
    return dep_int, extra_names, nextra


def data_layout(targets):
    """The visible data columns of a JointTarget's batch layout -> (ncols, {ref: slice}, {ref: obsx}): the hidden
    dispersion sources of an ellipticity target and the resampling scratch lie beyond ncols and are no data columns."""
    bl = targets.batch_layout(ell=True)
    desc, ncols = bl['desc'], bl['layout'].ncols
    where = {t.ref: slice(desc[n].off, desc[n].off + desc[n].n) for n, t in enumerate(targets.targets)}
    if ncols > _lib.DATACOV_MAX_S:
        raise ValueError("at most %d data columns (the targets have %d)" % (_lib.DATACOV_MAX_S, ncols))
    return ncols, where, {t.ref: np.asarray(t.obsdata.x) for t in targets.targets}


def summarize_sets(stations, models, set_start, vpvs, weights=None, dep_int=None, extra=None, extra_names=(), mantle=None,
                   device=None, rf_p=None, strict=True, max_rows=None):
    """summarize() of every set of rows: set s is models[set_start[s]:set_start[s + 1]] (set_start [sets + 1], ascending
    from 0 to the number of rows; a set may be empty) with its vpvs, weights and extra values, modelled for the
    JointTarget stations[s].

    stations   sequence of JointTargets that share targets and axes (StationPool's rule) -- and, with rf_p, differ in the
               ray parameter of their receiver functions
    rf_p       [stations, nrf] (stations.rf_slowness_table): every row is modelled at its own station's slowness
    max_rows   the sets are taken in runs of whole sets whose rows fit max_rows (default: what half of the free device
               memory holds): one forward pass, two segmented scans and one bh_datacov_sets call per run; no result
               depends on it

    -> a selection.SetList with summarize()'s dict per set, every field bit for bit what summarize returns for the set's
    rows alone.  A set for which summarize raises raises here too, as a ValueError naming the first such set -- or, with
    strict=False, has the entry None and its message in the list's `failed` {set index: message}.  A negative weight
    fails the call."""
    import torch
    stations = list(stations)
    dev, rows, w, _ = _device.device_rows(models, weights, None, device, per_row="one weight per row")
    R = rows.shape[0]
    set_start, Z = sel.check_set_start(set_start, R)
    if len(stations) != Z:
        raise ValueError("one JointTarget per set")
    dep_int, extra_names, nextra = check_columns(dep_int, extra, extra_names, R)
    vp = None if np.ndim(vpvs) == 0 else vpvs
    if vp is not None and len(vp) != R:
        raise ValueError("vpvs: one per row, or a scalar")
    if rf_p is not None and len(rf_p) != Z:
        raise ValueError("rf_p: one row of ray parameters per station")
    if max_rows is not None and int(max_rows) < 1:
        raise ValueError("max_rows >= 1")
    ncols, where, obsx = data_layout(stations[0])
    nd, K, names = dep_int.size, dep_int.size + nextra, column_names(dep_int, extra_names)
    results, failed = [None] * Z, {}
    if R == 0:
        failed = {z: "empty selection: no models" for z in range(Z)}
        sel.raise_first_failed(failed, strict, "set")
        return sel.SetList(results, failed)
    lib = _lib.load()
    E = None if not nextra else _device.to_device(extra, torch.float64, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if max_rows is None:           # half of the free device memory: the matrix of the modelled data and its flags
        bl = stations[0].batch_layout(ell=True)
        max_rows = max(1, int(torch.cuda.mem_get_info(dev)[0] // (2 * (bl['layout'].row * 8 + bl['nflags'] * 4))))
    for a, b in df.station_runs(set_start, max_rows):
        lo, hi = int(set_start[a]), int(set_start[b])
        if lo == hi:
            for z in range(a, b):
                failed[z] = "empty selection: no models"
            continue
        n, start = b - a, set_start[a:b + 1] - lo
        ids = None if rf_p is None else np.repeat(np.arange(a, b, dtype=np.int32), np.diff(start))
        with torch.cuda.device(dev):
            rw, ww, Ew = rows[lo:hi], None if w is None else w[lo:hi], None if E is None else E[lo:hi]
            _, Y, err, _ = df.forward_matrix(stations[a], rw, vpvs if vp is None else vp[lo:hi], mantle, dev, rf_p, ids)
            # a row without a model (fewer than two leading values) counts nowhere: weight 0 for the scan of the data
            nomodel = torch.isnan(rw[:, 1])
            wy = ww
            if bool(nomodel.any()):
                wy = torch.where(nomodel, 0, 1 if ww is None else ww).to(torch.int32)
            with post.Sets(rw, ww, None, start, dep_int, None, stream) as g:
                sx = g.scan()
            with ColumnScan(Y, ncols, wy, err, start, stream) as f:
                sy = f.scan()
                why = {i: f.status_text(sy['status'][i]) for i in range(n) if sy['status'][i]}
            live = (sx['status'] == 0) & (sy['status'] == 0)
            for i in np.nonzero(~live)[0]:
                failed[a + int(i)] = why[int(i)] if sx['status'][i] == 0 else \
                    lib.bh_posterior_sets_status_text(int(sx['status'][i])).decode()
            cx, constant_x = np.zeros((n, K)), np.zeros((n, K), dtype=bool)
            cx[:, :nd] = np.where(live[:, None], sx['mean'], 0.)
            constant_x[:, :nd] = sx['vmin'] == sx['vmax']
            if nextra:
                Em = Ew.clone()
                Em[nomodel] = float('nan')
                with ColumnScan(Em, nextra, ww, None, start, stream) as f:
                    se = f.scan()
                for i in np.nonzero(live)[0]:
                    if se['status'][i] != 0 or se['total'][i] != sx['total'][i]:
                        failed[a + int(i)] = "a NaN among the extra values"
                        live[i] = False
                cx[:, nd:] = np.where(live[:, None], se['mean'], 0.)
                constant_x[:, nd:] = se['vmin'] == se['vmax']
            cx[~live] = 0.
            cy = np.where(live[:, None], sy['mean'], 0.)
            m = datacov_sets(rw, ww, Ew, Y, ncols, err, start, dep_int, cx, cy, stream)
        for i in np.nonzero(live)[0]:
            W = int(m['total'][i])
            if W != sy['total'][i]:
                raise _lib.BayHunterAmdError("set %d: the scan of the data counted %d models, bh_datacov_sets %d"
                                             % (a + i, sy['total'][i], W))
            cov, corr, std_x, std_y = from_moments(m['C'][i], m['r1x'][i], m['r1y'][i], m['qx'][i], m['qy'][i], W,
                                                   constant_x[i], sy['vmin'][i] == sy['vmax'][i])
            # the centre of the model side is the mean over every row with a model; r1x / W is what it is off the mean
            # over the rows that count
            results[a + i] = dict(cov=cov, corr=corr, mean_x=cx[i] + m['r1x'][i] / W, std_x=std_x, mean_y=cy[i].copy(),
                                  std_y=std_y, names=list(names), targets=dict(where), x=dict(obsx), dep=dep_int,
                                  nmodels=W, nexcluded=int(m['excluded'][i]))
    sel.raise_first_failed(failed, strict, "set")
    return sel.SetList(results, failed)


def summarize(targets, models, vpvs, weights=None, dep_int=None, extra=None, extra_names=(), mantle=None, device=None):
    """Cross-covariance and correlation of the Vs(z) profile of `models` ([rows, 2*maxlayers], reference layout, float32
    or float64; numpy or a torch tensor) and their modelled data for the JointTarget `targets`, with vp/vs `vpvs` (one
    per row, or a scalar), integer `weights` (>= 0, default 1 each) and the prior's `mantle` (vs, vpvs) rule.

    dep_int      the depth grid (default posterior.default_dep_int(): 0.5 km steps to 100 km)
    extra        [rows, nextra] further model columns beside the depths (Vp/Vs, noise amplitudes), named by extra_names

    -> dict(cov, corr [K, S] (corr NaN in the row of a model column and in the column of a datum every model agrees on),
            mean_x, std_x [K], mean_y, std_y [S], names ('vs@<z>' per depth, then extra_names), targets {ref: the slice of
            the S data columns that is the target's}, x {ref: the target's obsdata.x}, dep, nmodels (weighted rows used),
            nexcluded (weighted rows left out: failed forward pass or NaN)), K = depths + nextra, S the visible
            columns of the targets' batch layout (`targets` says where each target's lie).
    ValueError for an empty selection."""
    nrows = models.shape[0] if len(models.shape) == 2 else 0
    res = summarize_sets([targets], models, [0, nrows], vpvs, weights, dep_int, extra, extra_names, mantle, device,
                         strict=False)
    if res[0] is None:
        raise ValueError(res.failed[0])
    return res[0]


# ---- chain pools ------------------------------------------------------------------------------------------

def extra_columns(pool, ci, ri, extras, device):
    """The columns `extras` of scalars.NAMES of the pool's rows as one contiguous device matrix (None: no extras)."""
    from . import scalars as sc
    extras = [str(e) for e in extras]
    names = sc.NAMES(pool.ntargets, [t.ref for t in pool.targets.targets])
    for e in extras:
        if e not in names:
            raise ValueError("extras: no column %r (there are %s)" % (e, ', '.join(names)))
    if not extras:
        return None, extras
    cols = sc.pool_columns(pool, ci, ri, None, device=device)
    return cols.data[:, [names.index(e) for e in extras]].contiguous(), extras


def pool_data_covariance(pool, dep_int=None, extras=('vpvs',), selection='weighted', dev=0.05, exclude_outliers=True,
                         device=None):
    """ChainPool.data_covariance: summarize() over the pool's main-phase rows (see ChainPool.data_covariance)."""
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    E, extras = extra_columns(pool, ci, ri, extras, device)
    res = summarize(pool.targets, pool.models[ci, ri], pool.vpvs[ci, ri].astype(np.float64), w.astype(np.int32), dep_int, E,
                    extras, pool.priors.get('mantle'), device)
    res['chains'] = np.unique(ci) + pool.first
    return res


class StationDataCovariance(sel.StationResult):
    """StationPool.data_covariance's result, every array in the pool's station order.

    names, failed    the stations; {station name: message} (such a station is NaN throughout)
    stations         {station name: the dict pool.station(name).data_covariance(...) returns}, failed stations left out
    columns, dep     the names of the K model columns ('vs@<z>' per depth, then the extras); the depth grid
    targets, x       {ref: the slice of the S data columns that is the target's}, {ref: the target's obsdata.x}
    cov, corr [nstations, K, S], mean_x, std_x [nstations, K], mean_y, std_y [nstations, S], nmodels, nexcluded
    [nstations] (0 for a failed station)"""

    def __init__(self, names, results, failed, columns, dep, targets, x, ncols):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {n: r for n, r in zip(names, results) if r is not None}
        self.columns, self.dep, self.targets, self.x = list(columns), dep, dict(targets), dict(x)
        Z, K, S = len(results), len(self.columns), int(ncols)
        self.cov, self.corr = np.full((Z, K, S), np.nan), np.full((Z, K, S), np.nan)
        self.mean_x, self.std_x = np.full((Z, K), np.nan), np.full((Z, K), np.nan)
        self.mean_y, self.std_y = np.full((Z, S), np.nan), np.full((Z, S), np.nan)
        self.nmodels, self.nexcluded = np.zeros(Z, dtype=np.int64), np.zeros(Z, dtype=np.int64)
        for z, r in enumerate(results):
            if r is not None:
                for k in ('cov', 'corr', 'mean_x', 'std_x', 'mean_y', 'std_y', 'nmodels', 'nexcluded'):
                    getattr(self, k)[z] = r[k]


def stations_data_covariance(spool, dep_int=None, extras=('vpvs',), selection='weighted', dev=0.05, exclude_outliers=True,
                             device=None, strict=True, max_rows=None):
    """StationPool.data_covariance: summarize_sets() over every station's main-phase rows, in runs of whole stations."""
    import torch
    pool, c = spool.pool, spool.chains_per_station
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    dep_int, _, _ = check_columns(dep_int, None, (), 0)
    ncols, where, obsx = data_layout(spool.stations[0])
    rf_p = None
    if 'p' in spool.per_station:
        from .stations import rf_slowness_table
        rf_p = rf_slowness_table(spool.stations)
    if max_rows is None:       # half of the free device memory: the modelled data and their flags, the model rows, the
        bl = spool.stations[0].batch_layout(ell=True)                                 # scalar columns, the weights
        per_row = bl['layout'].row * 8 + bl['nflags'] * 4 + 4 * pool.models.shape[2] + \
            8 * (3 * pool.ntargets + 4 + len(extras)) + 4
        max_rows = max(1, int(torch.cuda.mem_get_info(_device.torch_device(device))[0] // (2 * per_row)))
    results = []
    for a, b in df.station_runs(set_start, max_rows):
        lo, hi = int(set_start[a]), int(set_start[b])
        E, names = extra_columns(pool, ci[lo:hi], ri[lo:hi], extras, device)
        res = summarize_sets(spool.stations[a:b], pool.models[ci[lo:hi], ri[lo:hi]], set_start[a:b + 1] - lo,
                             pool.vpvs[ci[lo:hi], ri[lo:hi]].astype(np.float64), w[lo:hi].astype(np.int32), dep_int, E,
                             names, pool.priors.get('mantle'), device, None if rf_p is None else rf_p[a:b], strict=False,
                             max_rows=max_rows)
        results += list(res)
        for z, msg in res.failed.items():
            failed.setdefault(a + z, msg)
    sel.raise_first_failed(failed, strict, "station", spool.names)
    for z, r in enumerate(results):
        if r is not None:
            r['chains'] = sel.station_chains(ci, set_start, z, c)
    return StationDataCovariance(spool.names, results, failed, column_names(dep_int, [str(e) for e in extras]), dep_int,
                                 where, obsx, ncols)
