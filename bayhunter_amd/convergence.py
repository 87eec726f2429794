"""Convergence diagnostics on the device: split R-hat and the effective sample size, per pool and per station.

The reference shows convergence as traces that a person reads chain by chain (PlotFromStorage.plot_iiter*,
src/Plotting.py:317-435) and as get_outliers (:113-154; here ChainPool.outliers).  This module computes the two standard
numbers instead (Gelman et al., BDA3 section 11.4; Vehtari et al. 2021, without rank normalisation and without the
log10 cap): every chain's common main-phase window is split into two half chains, and

    split R-hat   compares the variance between the half chains' means with the variance inside them,
    ESS, tau      come from the autocorrelation of the half chains with Geyer's initial monotone sequence.

A half chain is a run-length coded series (selection.half_chain_series): every accepted row repeated once per iteration
it stayed current.  Its mean per column is the segmented column reduction of datafits (bh_datafits_sets_*, sets = half
chains); its autocovariance at lags 0 .. nlags - 1 is bh_autocov_sets (csrc/autocov.hip), the one part that depends on
the ORDER of a chain's rows.  What is left -- a few numbers per column -- is the pure functions below, which need no
device.
"""
import numpy as np

from . import _device, _lib, datafits as df, scalars as sc, selection as sel

FIELDS = ('rhat', 'ess', 'tau', 'truncated', 'constant', 'mean', 'W', 'B', 'var_plus')


# ---- the rules, without a device ------------------------------------------------------------------------

def geyer(rho):
    """Geyer's initial monotone sequence over the autocorrelations rho[0 .. T): P_k = rho[2k] + rho[2k + 1], cut at the
    first negative P_k, the kept ones made non-increasing -> (tau = -1 + 2 sum P, pairs kept, truncated: no P_k was
    negative among the T // 2 pairs, so tau is a lower bound).  NaN when P_0 < 0 or there is no pair."""
    rho = np.asarray(rho, dtype=np.float64)
    P = rho[0:rho.size // 2 * 2:2] + rho[1:rho.size // 2 * 2:2]
    if P.size == 0 or not np.all(np.isfinite(P)):
        return np.nan, 0, P.size == 0
    neg = np.nonzero(P < 0)[0]
    m = int(neg[0]) if neg.size else P.size
    if m == 0:
        return np.nan, 0, False
    return -1. + 2. * np.sum(np.minimum.accumulate(P[:m])), m, neg.size == 0


def diagnose(mean, acov, n, nlags=None):
    """Split R-hat, ESS and tau of one column from its M series of common length n: mean [M], acov [M, K] (divided by
    n, as bh_autocov_sets returns it).

        s_m^2 = acov_m[0] n / (n - 1),  W = mean_m s_m^2,  B = n var_m(mean_m) (ddof = 1),
        var+ = (n - 1) / n W + B / n,   rhat = sqrt(var+ / W),
        rho_t = 1 - (W - mean_m(acov_m[t] n / (n - 1))) / var+   for t < min(K, n),
        tau by geyer(rho),  ess = M n / tau

    -> dict(rhat, ess, tau, truncated, constant (W == 0: the diagnostics are NaN), mean (of the series' means), W, B,
            var_plus, acf [K] (rho up to the cut, NaN beyond))."""
    mean, acov = np.asarray(mean, dtype=np.float64), np.asarray(acov, dtype=np.float64)
    M, K = acov.shape
    n = int(n)
    if mean.shape != (M,) or M < 2 or n < 2:
        raise ValueError("diagnose: mean [M], acov [M, K] of M >= 2 series of n >= 2 samples")
    K = K if nlags is None else min(K, int(nlags))
    scale = n / (n - 1.)
    W = np.mean(acov[:, 0] * scale)
    B = n * np.var(mean, ddof=1)
    vp = (n - 1.) / n * W + B / n
    out = dict(rhat=np.nan, ess=np.nan, tau=np.nan, truncated=False, constant=bool(W == 0), mean=np.mean(mean), W=W, B=B,
               var_plus=vp, acf=np.full(acov.shape[1], np.nan))
    if not W > 0 or not np.isfinite(vp):
        return out
    out['rhat'] = np.sqrt(vp / W)
    T = min(K, n)
    rho = 1. - (W - np.mean(acov[:, :T] * scale, axis=0)) / vp
    tau, kept, trunc = geyer(rho)
    out['acf'][:2 * kept] = rho[:2 * kept]
    out.update(tau=tau, truncated=bool(trunc), ess=M * n / tau)
    return out


def group_diagnostics(mean, acov, n, names):
    """diagnose() of every column of one group: mean [M, C], acov [M, C, K], series 2i and 2i + 1 the two halves of
    chain i -> {name: diagnose's dict plus tau_chain, ess_chain [M / 2] (the same from each chain's own two halves)}."""
    mean, acov = np.asarray(mean, dtype=np.float64), np.asarray(acov, dtype=np.float64)
    M = mean.shape[0]
    if M % 2 or M < 2:
        raise ValueError("a group is the two half chains of each of its chains")
    out = {}
    for c, name in enumerate(names):
        d = diagnose(mean[:, c], acov[:, c], n)
        per = [diagnose(mean[i:i + 2, c], acov[i:i + 2, c], n) for i in range(0, M, 2)]
        d['tau_chain'] = np.array([p['tau'] for p in per])
        d['ess_chain'] = np.array([p['ess'] for p in per])
        out[name] = d
    return out


def converged(d, chains, rhat_max=1.01, ess_min=None):
    """The verdict on one column's dict: rhat <= rhat_max, ess >= ess_min (default 100 per chain, Vehtari et al.'s
    recommendation: a policy, not a measurement) and the sum of the autocorrelations not truncated."""
    ess_min = 100. * chains if ess_min is None else ess_min
    return bool(d['rhat'] <= rhat_max and d['ess'] >= ess_min and not d['truncated'])


# ---- on the device ------------------------------------------------------------------------------------------

def autocov_sets(M, weights, series_start, mean, nlags, stream):
    """bh_autocov_sets over the device matrix M [rows, K] (weights: int32 device tensor or None) -> (acov [series, K,
    nlags], length [series])."""
    series_start = np.ascontiguousarray(series_start, dtype=np.int64)
    S, K = series_start.size - 1, M.shape[1]
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    if mean.shape != (S, K):
        raise ValueError("mean: [series, columns]")
    acov = np.zeros((S, K, int(nlags)))
    length = np.zeros(S, dtype=np.int64)
    _lib.check(_lib.load().bh_autocov_sets(M.data_ptr(), M.shape[0], M.stride(0), K, None if weights is None else
                                           weights.data_ptr(), series_start.ctypes.data, S, mean.ctypes.data, int(nlags),
                                           acov.ctypes.data, length.ctypes.data, stream))
    return acov, length


def summarize(cols, weights, series_start, group_start, nlags=1024, device=None):
    """The diagnostics of every group of series: `cols` a scalars.Columns whose rows are the entries of the series
    (its 'pair' columns are left out), `weights` their integer weights (None: 1 each), series s the rows
    series_start[s]:series_start[s + 1], group g the series group_start[g]:group_start[g + 1] -- the two half chains of
    each of its chains, all of one length.

    One segmented reduction for the series' means and one bh_autocov_sets launch with those means; the rest on the host
    (group_diagnostics).  -> a SetList: per group dict(<column>: diagnose's dict with tau_chain, ess_chain; n, nseries),
    None for a group in `failed`: no series, or a NaN in a column -- the reduction leaves a row with a NaN out of every
    column's mean, so such a group has no mean to centre any of its columns on.  ValueError for a group whose series differ in length."""
    import torch
    if not isinstance(cols, sc.Columns):
        raise ValueError("cols: a scalars.Columns")
    if not 1 <= int(nlags) <= _lib.AUTOCOV_MAX_LAGS:
        raise ValueError("nlags: 1 to %d" % _lib.AUTOCOV_MAX_LAGS)
    K, names = cols.nstat, cols.names[:cols.nstat]
    R = cols.data.shape[0]
    series_start, S = sel.check_set_start(series_start, R)
    group_start, G = sel.check_set_start(group_start, S)
    if weights is not None and len(weights) != R:
        raise ValueError("one weight per row")
    results, failed = [None] * G, {}
    if R == 0:
        return sel.SetList(results, {g: "empty selection: no rows" for g in range(G)})
    dev = _device.torch_device(device)
    M = _device.to_device(cols.data, torch.float64, dev)[:, :K]
    if M.stride(1) != 1:
        M = M.contiguous()
    w = None if weights is None else _device.to_device(weights, torch.int32, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        with df._FitsSets(M, K, w, None, series_start, stream) as f:
            s = f.scan()
        mean = np.where((s['status'] == 0)[:, None], s['mean'], 0.)
        acov, length = autocov_sets(M, w, series_start, mean, nlags, stream)
    for g in range(G):
        a, b = int(group_start[g]), int(group_start[g + 1])
        if a == b:
            failed[g] = "empty selection: no series"
            continue
        n = length[a:b]
        if np.any(n != n[0]):
            raise ValueError("group %d: its series differ in length (%d to %d)" % (g, n.min(), n.max()))
        if np.any(s['excluded'][a:b] > 0) or np.any(s['status'][a:b] != 0):
            failed[g] = "a NaN in a column, or a series without rows"
            continue
        d = group_diagnostics(mean[a:b], acov[a:b], int(n[0]), names)
        d.update(n=int(n[0]), nseries=b - a)
        results[g] = d
    return sel.SetList(results, failed)


# ---- chain pools ------------------------------------------------------------------------------------------

def vs_at(models, depths):
    """The Vs of the layer that holds each depth, per reference-layout row (vs | z of the nuclei, NaN beyond): the
    interfaces are the float64 midpoints of neighbouring nuclei (posterior.stepmodel's layering), a depth on an interface
    belongs to the layer below -> [rows, len(depths)]."""
    models = np.asarray(models, dtype=np.float64)
    R, maxn = models.shape[0], models.shape[1] // 2
    n = (~np.isnan(models)).sum(axis=1) // 2
    k = np.arange(maxn)[None, :]
    with np.errstate(invalid='ignore'):
        z = np.take_along_axis(models, np.minimum(n[:, None] + k, models.shape[1] - 1), axis=1)
        z = np.where(k < n[:, None], z, np.nan)
        mid = (z[:, :-1] + z[:, 1:]) / 2.
        out = np.empty((R, len(depths)))
        for i, d in enumerate(depths):
            layer = (mid <= np.float64(d)).sum(axis=1)
            out[:, i] = models[np.arange(R), layer]
    return out


def columns(pool, ci, ri, depths=(), device=None):
    """scalars.pool_columns of the rows (without moho) and one float64 column 'vs@<z>' per depth of `depths`."""
    import torch
    cols = sc.pool_columns(pool, ci, ri, None, device=device)
    if not len(depths):
        return cols
    extra = _device.to_device(vs_at(pool.models[ci, ri], depths), torch.float64, cols.data.device)
    return sc.Columns(torch.cat((cols.data, extra), dim=1), cols.tags + [sc.F8] * len(depths),
                      cols.names + ['vs@%g' % float(d) for d in depths])


def _groups(pool, c, nlags, depths, dev, exclude_outliers, rhat_max, ess_min, device, max_rows, global_chains):
    """half_chain_series and summarize() in runs of whole groups -> (per group its dict or None, failed).  global_chains:
    'chains' are the pool's global indices (the whole pool is the group), else indices within the group (a station)."""
    import torch
    hs = sel.half_chain_series(pool, c, dev, exclude_outliers)
    failed = dict(hs['failed'])
    gs, ss = hs['group_start'], hs['series_start']
    G = gs.size - 1
    entry_start = ss[gs]
    ncols = 3 * pool.ntargets + 4 + len(depths)
    if max_rows is None:           # half of the free device memory: the matrix, the weights and their prefix sum
        max_rows = max(1, int(torch.cuda.mem_get_info(_device.torch_device(device))[0] // (2 * (8 * ncols + 12))))
    most = max(1, (1 << 30) // (2 * c * ncols * int(nlags) * 8))         # groups whose autocovariances take 1 GiB
    results = [None] * G
    for first, last in df.station_runs(entry_start, max_rows):
        for a in range(first, last, most):
            e = min(last, a + most)
            lo, hi = int(entry_start[a]), int(entry_start[e])
            if lo == hi:
                continue
            cols = columns(pool, hs['ci'][lo:hi], hs['ri'][lo:hi], depths, device)
            res = summarize(cols, hs['w'][lo:hi].astype(np.int32), ss[gs[a]:gs[e] + 1] - lo, gs[a:e + 1] - gs[a], nlags,
                            device)
            for g in range(a, e):
                if res[g - a] is None:
                    failed.setdefault(g, res.failed[g - a])
                    continue
                d = res[g - a]
                chains = hs['chains'][gs[g] // 2:gs[g + 1] // 2]
                for name in list(d):
                    if isinstance(d[name], dict):
                        d[name]['converged'] = converged(d[name], chains.size, rhat_max, ess_min)
                d.update(chains=chains + pool.first if global_chains else chains - g * c, window=tuple(int(v) for v in hs['window'][g]),
                         first_iter=hs['first_iter'][chains])
                results[g] = d
    return results, failed


def pool_convergence(pool, nlags=1024, depths=(), dev=0.05, exclude_outliers=True, rhat_max=1.01, ess_min=None, device=None):
    """ChainPool.convergence: the whole pool is one group."""
    results, failed = _groups(pool, pool.nchains, nlags, depths, dev, exclude_outliers, rhat_max, ess_min, device, None,
                              True)
    if results[0] is None:
        raise ValueError(failed[0])
    return results[0]


class StationConvergence(sel.StationResult):
    """StationPool.convergence's result, every array in the pool's station order.

    names, failed    the stations; {station name: message} (such a station is a row of NaN)
    stations         {station name: the dict pool.station(name).convergence(...) returns}, failed stations left out
    columns          the names of the columns
    rhat, ess, tau, truncated, converged    {column: [nstations]} (float64; NaN for a failed station)
    window           [nstations, 2] the common main-phase window of the station's chains (-1 for a failed station)"""

    STACKED = ('rhat', 'ess', 'tau', 'truncated', 'converged')

    def __init__(self, names, results, failed):
        sel.StationResult.__init__(self, names, failed)
        self.stations = {n: r for n, r in zip(names, results) if r is not None}
        first = next((r for r in results if r is not None), None)
        self.columns = [] if first is None else [k for k, v in first.items() if isinstance(v, dict)]
        for k in self.STACKED:
            setattr(self, k, {c: np.array([np.nan if r is None else float(r[c][k]) for r in results])
                              for c in self.columns})
        self.window = np.array([(-1, -1) if r is None else r['window'] for r in results], dtype=np.int64).reshape(-1, 2)


def stations_convergence(spool, nlags=1024, depths=(), dev=0.05, exclude_outliers=True, rhat_max=1.01, ess_min=None,
                         device=None, strict=True, max_rows=None):
    """StationPool.convergence: every station a group, in runs of whole stations."""
    results, failed = _groups(spool.pool, spool.chains_per_station, nlags, depths, dev, exclude_outliers, rhat_max,
                              ess_min, device, max_rows, False)
    sel.raise_first_failed(failed, strict, "station", spool.names)
    return StationConvergence(spool.names, results, failed)
