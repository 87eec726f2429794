"""Posterior covariance and correlation of the Vs(z) profile, on the device: how Vs at one depth moves with Vs at another.

Every other statistic of the package describes one depth or one scalar.  This one is the second moment of the whole
profile -- the velocity / thickness trade-off around an interface, the anti-correlation of neighbouring layers, the depth
range a receiver function pins, the correlation length of the mean -+ std band -- and, with a few scalar columns beside
the depths (Vp/Vs, noise amplitudes), the Vs - Vp/Vs trade-off per depth.  The reference leaves it to the eye.

Every row carries an integer weight; the result equals np.cov(X.T, bias=True) on the matrix X in which each row's Vs on
the depth grid (and its extra values) is repeated `weight` times, without building that matrix.  The means are the
segmented scan's (posterior.Sets.scan; for the extra columns the segmented column reduction that scalars uses); the one
new device part is bh_depthcov_sets (csrc/depthcov.hip): per set S = sum w d d^T and r1 = sum w d over the rows centred
on those means, on the FP64 matrix cores.  What is left is from_moments() below, which needs no device.
"""
import numpy as np

from . import _device, _lib, datafits as df, posterior as post, selection as sel

BUDGET_BYTES = 1 << 30       # of the S matrices of one bh_depthcov_sets call (summarize_sets' `budget_bytes`)


# ---- the rules, without a device ------------------------------------------------------------------------

def from_moments(S, r1, W, constant=None):
    """Covariance, correlation and standard deviation from the centred moments of one set: S [K, K] = sum w d d^T,
    r1 [K] = sum w d, W = sum w, d = x - c for ANY centre c:

        cov = (S - r1 r1^T / W) / W      (population, np.cov(..., bias=True); r1 takes out what c is off the mean)
        std = sqrt(diag cov),  corr = cov / (std std^T)

    constant [K] marks columns known to hold one value (their min equals their max): their variance is exactly 0, whatever
    the rounding of c left in S.  A column of variance 0 has std 0, covariance 0 and a NaN row and column in corr.
    -> (cov, corr, std)."""
    S, r1 = np.asarray(S, dtype=np.float64), np.asarray(r1, dtype=np.float64)
    K = r1.size
    if S.shape != (K, K) or not W > 0:
        raise ValueError("from_moments: S [K, K], r1 [K] and a weight total above 0")
    W = float(W)
    cov = (S - np.outer(r1, r1) / W) / W
    var = np.diagonal(cov).copy()
    flat = var <= 0
    if constant is not None:
        flat |= np.asarray(constant, dtype=bool)
    cov[flat, :] = 0.
    cov[:, flat] = 0.
    var[flat] = 0.
    std = np.sqrt(var)
    with np.errstate(invalid='ignore', divide='ignore'):
        corr = cov / np.outer(std, std)
    corr[flat, :] = np.nan
    corr[:, flat] = np.nan
    live = ~flat & ~np.isnan(var)
    corr[live, live] = 1.
    return cov, corr, std


def column_names(dep_int, extra_names=()):
    """'vs@<z>' per depth, as convergence() names its depth columns, then the extra columns' names."""
    return ['vs@%g' % float(d) for d in dep_int] + [str(n) for n in extra_names]


# ---- on the device ------------------------------------------------------------------------------------------

def depthcov_sets(rows, weights, extra, set_start, dep, center, stream):
    """bh_depthcov_sets over device rows (weights: int32 device tensor or None; extra: float64 device matrix or None)
    -> (S [sets, K, K], r1 [sets, K], total [sets])."""
    set_start = np.ascontiguousarray(set_start, dtype=np.int64)
    dep = np.ascontiguousarray(dep, dtype=np.float64)
    Z, nextra = set_start.size - 1, 0 if extra is None else extra.shape[1]
    K = dep.size + nextra
    center = np.ascontiguousarray(center, dtype=np.float64)
    if center.shape != (Z, K):
        raise ValueError("center: [sets, depths + extra columns]")
    S, r1, total = np.zeros((Z, K, K)), np.zeros((Z, K)), np.zeros(Z, dtype=np.int64)
    _lib.check(_lib.load().bh_depthcov_sets(
        rows.data_ptr(), int(rows.dtype.itemsize == 8), rows.shape[0], rows.stride(0), rows.shape[1],
        None if weights is None else weights.data_ptr(), None if extra is None else extra.data_ptr(),
        0 if extra is None else extra.stride(0), nextra, set_start.ctypes.data, Z, dep.ctypes.data, dep.size,
        center.ctypes.data, S.ctypes.data, r1.ctypes.data, total.ctypes.data, stream))
    return S, r1, total


def _check(dep_int, extra, extra_names, nrows):
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


def summarize_sets(models, set_start, weights=None, dep_int=None, extra=None, extra_names=(), device=None, strict=True,
                   budget_bytes=BUDGET_BYTES):
    """summarize() of every set of rows: set s is models[set_start[s]:set_start[s + 1]] (set_start [sets + 1], ascending
    from 0 to the number of rows; a set may be empty), with its weights and extra values.  One segmented scan for the
    means and one bh_depthcov_sets call for all sets.

    -> a selection.SetList with summarize()'s dict per set, every field bit for bit what summarize returns for the set's
    rows alone.  A set for which summarize raises (no row of positive weight with a model; a NaN among its extra values)
    raises here too, as a ValueError naming the first such set -- or, with strict=False, has the entry None and its
    message in the list's `failed` {set index: message}.  A negative weight fails the call.

    budget_bytes   bound on the S matrices of one call, sets * K^2 * 8 bytes (default 1 GiB; 1 024 sets of 201 depths are
                   331 MB): the sets are taken in runs of whole sets that keep to it, and no result depends on it."""
    import torch
    dev, rows, w, _ = _device.device_rows(models, weights, None, device, per_row="one weight per row")
    R = rows.shape[0]
    set_start, Z = sel.check_set_start(set_start, R)
    dep_int, extra_names, nextra = _check(dep_int, extra, extra_names, R)
    if int(budget_bytes) < 1:
        raise ValueError("budget_bytes >= 1")
    K, names = dep_int.size + nextra, column_names(dep_int, extra_names)
    results, failed = [None] * Z, {}
    if R == 0:
        failed = {z: "empty selection: no models" for z in range(Z)}
        sel.raise_first_failed(failed, strict, "set")
        return sel.SetList(results, failed)
    lib = _lib.load()
    E = None if not nextra else _device.to_device(extra, torch.float64, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    center, constant = np.zeros((Z, K)), np.zeros((Z, K), dtype=bool)
    S, r1, total = np.zeros((Z, K, K)), np.zeros((Z, K)), np.zeros(Z, dtype=np.int64)
    with torch.cuda.device(dev):
        with post.Sets(rows, w, None, set_start, dep_int, None, stream) as g:
            s = g.scan()
        live = s['status'] == 0
        for z in np.nonzero(~live)[0]:
            failed[int(z)] = lib.bh_posterior_sets_status_text(int(s['status'][z])).decode()
        center[:, :dep_int.size] = np.where(live[:, None], s['mean'], 0.)
        constant[:, :dep_int.size] = s['vmin'] == s['vmax']
        if nextra:
            # the extra columns' means over the rows the scan counts: a row without a model (fewer than two leading
            # values) is a row of NaN to the column reduction, which leaves such a row out
            Em = E.clone()
            Em[torch.isnan(rows[:, 1])] = float('nan')
            with df._FitsSets(Em, nextra, w, None, set_start, stream) as f:
                se = f.scan()
            for z in np.nonzero(live)[0]:
                if se['status'][z] != 0 or se['total'][z] != s['total'][z]:
                    failed[int(z)] = "a NaN among the extra values"
                    live[z] = False
            center[:, dep_int.size:] = np.where(live[:, None], se['mean'], 0.)
            constant[:, dep_int.size:] = se['vmin'] == se['vmax']
        center[~live] = 0.
        for a, b in df.station_runs(np.arange(Z + 1), max(1, int(budget_bytes) // (8 * K * K))):     # runs of that many sets
            lo, hi = int(set_start[a]), int(set_start[b])
            if lo == hi:
                continue
            S[a:b], r1[a:b], total[a:b] = depthcov_sets(rows[lo:hi], None if w is None else w[lo:hi],
                                                        None if E is None else E[lo:hi], set_start[a:b + 1] - lo, dep_int,
                                                        center[a:b], stream)
    for z in np.nonzero(live)[0]:
        if total[z] != s['total'][z]:
            raise _lib.BayHunterAmdError("set %d: the scan counted %d models, bh_depthcov_sets %d"
                                         % (z, s['total'][z], total[z]))
        cov, corr, std = from_moments(S[z], r1[z], int(total[z]), constant[z])
        results[z] = dict(cov=cov, corr=corr, mean=center[z].copy(), std=std, names=list(names), nmodels=int(total[z]),
                          dep=dep_int)
    sel.raise_first_failed(failed, strict, "set")
    return sel.SetList(results, failed)


def summarize(models, weights=None, dep_int=None, extra=None, extra_names=(), device=None):
    """Covariance and correlation of the Vs(z) profile of `models` ([rows, 2*maxlayers], reference layout, float32 or
    float64; numpy or a torch tensor) with integer `weights` (>= 0, default 1 each).

    dep_int      the depth grid (default posterior.default_dep_int(): 0.5 km steps to 100 km)
    extra        [rows, nextra] further columns beside the depths (Vp/Vs, noise amplitudes), named by extra_names

    -> dict(cov [K, K], corr [K, K] (NaN in the rows and columns of a variance of 0), mean [K], std [K] (0 there),
            names ('vs@<z>' per depth, then extra_names), nmodels (the weight total), dep), K = depths + nextra: what
            np.cov(X.T, bias=True) and np.corrcoef(X.T) give on the matrix X of the expanded rows.
    ValueError for an empty selection."""
    nrows = models.shape[0] if len(models.shape) == 2 else 0
    res = summarize_sets(models, [0, nrows], weights, dep_int, extra, extra_names, device, strict=False)
    if res[0] is None:
        raise ValueError(res.failed[0])
    return res[0]


# ---- chain pools ------------------------------------------------------------------------------------------

def _extra_columns(pool, ci, ri, extras, device):
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


def pool_depth_covariance(pool, dep_int=None, extras=('vpvs',), selection='weighted', dev=0.05, exclude_outliers=True,
                          device=None):
    """ChainPool.depth_covariance: summarize() over the pool's main-phase rows (see ChainPool.depth_covariance)."""
    ci, ri, w = sel.pool_rows(pool, selection, dev, exclude_outliers)
    E, extras = _extra_columns(pool, ci, ri, extras, device)
    res = summarize(pool.models[ci, ri], w.astype(np.int32), dep_int, E, extras, device)
    res['chains'] = np.unique(ci) + pool.first
    return res


class StationDepthCovariance(sel.StationResult):
    """StationPool.depth_covariance's result, every array in the pool's station order.

    names, failed    the stations; {station name: message} (such a station is NaN throughout)
    stations         {station name: the dict pool.station(name).depth_covariance(...) returns}, failed stations left out
    columns, dep     the names of the K columns ('vs@<z>' per depth, then the extras); the depth grid
    cov, corr [nstations, K, K], mean, std [nstations, K], nmodels [nstations] (0 for a failed station)"""

    def __init__(self, names, results, failed, columns, dep):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {n: r for n, r in zip(names, results) if r is not None}
        self.columns, self.dep = list(columns), dep
        Z, K = len(results), len(self.columns)
        self.cov, self.corr = np.full((Z, K, K), np.nan), np.full((Z, K, K), np.nan)
        self.mean, self.std = np.full((Z, K), np.nan), np.full((Z, K), np.nan)
        self.nmodels = np.zeros(Z, dtype=np.int64)
        for z, r in enumerate(results):
            if r is not None:
                self.cov[z], self.corr[z], self.mean[z], self.std[z] = r['cov'], r['corr'], r['mean'], r['std']
                self.nmodels[z] = r['nmodels']


def stations_depth_covariance(spool, dep_int=None, extras=('vpvs',), selection='weighted', dev=0.05, exclude_outliers=True,
                              device=None, strict=True, max_rows=None, budget_bytes=BUDGET_BYTES):
    """StationPool.depth_covariance: summarize_sets() over every station's main-phase rows, in runs of whole stations."""
    import torch
    pool, c = spool.pool, spool.chains_per_station
    ci, ri, w, set_start, failed = sel.station_rows(pool, c, selection, dev, exclude_outliers)
    dep_int, _, _ = _check(dep_int, None, (), 0)
    if max_rows is None:       # half of the free device memory: the model rows, the scalar columns, the weights
        per_row = 4 * pool.models.shape[2] + 8 * (3 * pool.ntargets + 4 + len(extras)) + 4
        max_rows = max(1, int(torch.cuda.mem_get_info(_device.torch_device(device))[0] // (2 * per_row)))
    results = []
    for a, b in df.station_runs(set_start, max_rows):
        lo, hi = int(set_start[a]), int(set_start[b])
        E, names = _extra_columns(pool, ci[lo:hi], ri[lo:hi], extras, device)
        res = summarize_sets(pool.models[ci[lo:hi], ri[lo:hi]], set_start[a:b + 1] - lo, w[lo:hi].astype(np.int32), dep_int,
                             E, names, device, strict=False, budget_bytes=budget_bytes)
        results += list(res)
        for z, msg in res.failed.items():
            failed.setdefault(a + z, msg)
    sel.raise_first_failed(failed, strict, "station", spool.names)
    for z, r in enumerate(results):
        if r is not None:
            r['chains'] = sel.station_chains(ci, set_start, z, c)
    return StationDepthCovariance(spool.names, results, failed, column_names(dep_int, [str(e) for e in extras]), dep_int)
