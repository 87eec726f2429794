"""Which rows of a chain pool every statistic reads, in which sets, and what became of a set that has none: plain
numpy on the pool's host arrays, shared by posterior, datafits and moho."""
import numpy as np


def check_set_start(set_start, nrows):
    """-> (set_start as contiguous int64 [sets + 1], sets); ValueError unless it ascends from 0 to nrows."""
    set_start = np.ascontiguousarray(set_start, dtype=np.int64)
    S = set_start.size - 1
    if set_start.ndim != 1 or S < 1 or set_start[0] != 0 or set_start[-1] != nrows or np.any(np.diff(set_start) < 0):
        raise ValueError("set_start: [sets + 1], ascending from 0 to the number of rows")
    return set_start, S


def raise_first_failed(failed, strict, what, names=None):
    """strict: the first set (station, with `names`) of `failed` {index: message} is a ValueError."""
    if failed and strict:
        z = min(failed)
        raise ValueError(("%s %r: %s" if names else "%s %d: %s") % (what, names[z] if names else z, failed[z]))


class SetList(list):
    """A per-set result list: entry s is the dict of set s, or None for a set in `failed` ({set index: message})."""

    def __init__(self, results, failed):
        list.__init__(self, results)
        self.failed = failed


class StationResult(object):
    """What every StationPool statistic reports: `names` (the pool's stations) and `failed` {station name: message}."""

    def __init__(self, names, failed):
        self.names = list(names)
        self.failed = {names[z]: msg for z, msg in failed.items()}


# ---- the chain pool's own sample block ------------------------------------------------------------------

def pool_selection(pool, selection='weighted'):
    """Main-phase rows of a pool without a per-chain loop -> (chain index [rows] (local), row index [rows],
    weight [rows] int64).  'weighted': residence time, ChainPool.weighted (next row's iter, or iter_main, minus
    this row's).  'saved': how many of the rows save() writes are this row -- a row spanning the expanded
    range [a, a + w) of its chain contributes ceil((a + w) / t) - ceil(a / t) rows at thinning t."""
    if selection not in ('weighted', 'saved'):
        raise ValueError("selection: 'weighted' or 'saved'")
    n = np.asarray(pool.counters()[0], dtype=np.int64)
    it = pool.iter
    with np.errstate(invalid='ignore'):
        main = (np.arange(it.shape[1])[None, :] < n[:, None]) & (it >= 0)
    ci, ri = np.nonzero(main)
    if ci.size == 0:
        return ci, ri, np.zeros(0, dtype=np.int64)
    iv = it[ci, ri].astype(np.int64)
    last = np.r_[ci[1:] != ci[:-1], True]
    nxt = np.r_[iv[1:], 0]
    nxt[last] = pool.iter_main
    w = nxt - iv
    if selection == 'saved':
        first = np.r_[True, ci[1:] != ci[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(ci.size), 0))
        a = iv - iv[start]
        total = pool.iter_main - iv[start]
        t = -(-total // int(pool.initparams['maxmodels']))
        w = -(-(a + w) // t) - (-(-a // t))
    return ci, ri, w


def chain_like_medians(pool):
    """The median of each chain's thinned main-phase likes, as np.median of the float32 values save() writes gives it
    -> (chains (local indices of those with main-phase rows, ascending), medians float64)."""
    ci, ri, cnt = pool_selection(pool, 'saved')
    if ci.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0)
    likes = pool.likes[ci, ri]
    order = np.lexsort((likes, ci))
    cs, ls = cnt[order], likes[order]
    cum = np.cumsum(cs)
    chains = np.unique(ci)
    tot = np.bincount(ci, weights=cnt, minlength=pool.nchains).astype(np.int64)[chains]
    off = np.concatenate(([0], np.cumsum(tot)[:-1]))
    pick = lambda r: ls[np.searchsorted(cum, off + r, side='right')]
    lo, hi = pick((tot - 1) // 2), pick(tot // 2)
    # np.median of float32: the middle value, or the float32 mean of the two middle ones
    return chains, np.where(tot % 2 == 1, lo, (lo + hi) / np.float32(2)).astype(np.float32).astype(np.float64)


_NO_BEST_CHAIN = "best chain median likelihood is 0: outliers are undefined (Plotting.py:136-140)"


def pool_outliers(pool, dev=0.05):
    """PlotFromStorage.get_outliers (Plotting.py:113-154) on the likes save() writes: the median of each
    chain's thinned main-phase likes against the best chain's -> global chain indices (sorted)."""
    chains, med = chain_like_medians(pool)
    if chains.size == 0:
        return np.zeros(0, dtype=np.int64)
    maxlike = np.max(med)
    if maxlike > 0:
        scores = med / maxlike
    elif maxlike < 0:
        scores = maxlike / med
    else:
        raise ValueError(_NO_BEST_CHAIN)
    return (chains[(1 - scores) > dev] + pool.first).astype(np.int64)


def pool_rows(pool, selection='weighted', dev=0.05, exclude_outliers=True):
    """The rows ChainPool.posterior and ChainPool.datafits summarize: pool_selection without the outlier chains
    -> (ci, ri, w).  ValueError when nothing is left or a weight does not fit the device's int32."""
    ci, ri, w = pool_selection(pool, selection)
    if exclude_outliers and ci.size:
        out = pool_outliers(pool, dev) - pool.first
        keep = ~np.isin(ci, out)
        ci, ri, w = ci[keep], ri[keep], w[keep]
    if ci.size == 0:
        raise ValueError("empty selection: no main-phase rows")
    if w.max() > np.iinfo(np.int32).max:
        raise ValueError("a weight above 2^31 - 1")
    return ci, ri, w


# ---- every station of a station pool ----------------------------------------------------------------------

def station_rows(pool, chains_per_station, selection='weighted', dev=0.05, exclude_outliers=True):
    """pool_rows of every station of a pool whose chains come in runs of `chains_per_station` per station, without
    a loop over stations: the selection is pool_selection on all chains, the outlier chains are found per station
    from chain_like_medians on all chains (each chain's median against the best of its own station).
    -> (ci, ri, w, set_start [stations + 1], failed {station index: message}): station s owns the rows
    set_start[s]:set_start[s + 1], there ci - s * chains_per_station, ri, w are pool_rows of the station's view.
    A station in `failed` (its best chain's median likelihood is 0, or a weight does not fit the device's int32: what
    pool_rows raises for) has no rows; so has one without main-phase rows."""
    c = int(chains_per_station)
    S = pool.nchains // c
    ci, ri, w = pool_selection(pool, selection)
    failed = {}
    if exclude_outliers and ci.size:
        chains, med = chain_like_medians(pool)
        st = chains // c
        best = np.full(S, -np.inf)
        np.maximum.at(best, st, med)
        best = best[st]
        with np.errstate(divide='ignore', invalid='ignore'):
            scores = np.where(best > 0, med / best, best / med)
        for s in np.unique(st[best == 0]):
            failed[int(s)] = _NO_BEST_CHAIN
        out = chains[(best != 0) & ((1 - scores) > dev)]
        keep = ~np.isin(ci, out) & ~np.isin(ci // c, np.fromiter(failed, dtype=np.int64, count=len(failed)))
        ci, ri, w = ci[keep], ri[keep], w[keep]
    big = w > np.iinfo(np.int32).max
    if big.any():                                          # pool_rows' refusal, for the stations it would refuse
        for s in np.unique(ci[big] // c):
            failed.setdefault(int(s), "a weight above 2^31 - 1")
        keep = ~np.isin(ci // c, np.unique(ci[big] // c))
        ci, ri, w = ci[keep], ri[keep], w[keep]
    return ci, ri, w, np.searchsorted(ci // c, np.arange(S + 1)).astype(np.int64), failed


def station_chains(ci, set_start, z, chains_per_station):
    """The chains station z's rows come from, as indices into the station's own view (station_rows' ci, set_start)."""
    return np.unique(ci[set_start[z]:set_start[z + 1]]) - z * chains_per_station


# ---- the order of a chain's rows: half chains for the convergence diagnostics ------------------------------

def half_chain_series(pool, chains_per_group, dev=0.05, exclude_outliers=True):
    """The two half chains of every chain, group by group (a group: `chains_per_group` consecutive chains -- the whole
    pool, or one station), as run-length coded series for split R-hat and the effective sample size.

    Per group the chains are the ones station_rows takes with selection='weighted' (those of pool_rows for a group
    that is the whole pool).  Their common window is [t0, iter_main), t0 the latest first main-phase iteration among
    them: a chain that accepts late shortens its group's window.  With n = (iter_main - t0) // 2 the half windows are
    [iter_main - 2n, iter_main - n) and [iter_main - n, iter_main); a row enters a half with the iterations it spends
    inside it, so a row that straddles the boundary is in both halves with its share of the weight, and one that begins
    before the window is clipped.  Every series then has exactly n samples.

    -> dict(ci, ri, w [entries] (int64; the series one after the other: chain by chain, first half then second half),
            series_start [series + 1] (entries), group_start [groups + 1] (series), chains [series / 2] (the chain of
            each pair of series, a pool-local index), n [groups], window [groups, 2] = (iter_main - 2n, iter_main)
            (-1 for a failed group), first_iter [nchains] (the first main-phase iteration of every chain that has series;
            -1 for the others: no main-phase row, left out as an outlier, or of a group station_rows failed),
            failed {group: message}).
    A group in `failed` -- station_rows' reasons, no chain left, or n < 4 -- has no entries."""
    c = int(chains_per_group)
    G = pool.nchains // c
    ci, ri, w, set_start, failed = station_rows(pool, c, 'weighted', dev, exclude_outliers)
    failed = dict(failed)
    iv = pool.iter[ci, ri].astype(np.int64)
    first = np.r_[True, ci[1:] != ci[:-1]] if ci.size else np.zeros(0, dtype=bool)
    first_iter = np.full(pool.nchains, -1, dtype=np.int64)
    first_iter[ci[first]] = iv[first]
    n = np.zeros(G, dtype=np.int64)
    window = np.full((G, 2), -1, dtype=np.int64)
    end = int(pool.iter_main)
    for g in range(G):
        if g in failed:
            continue
        used = np.unique(ci[set_start[g]:set_start[g + 1]])
        if used.size == 0:
            failed[g] = "empty selection: no main-phase rows"
            continue
        n[g] = (end - int(first_iter[used].max())) // 2
        if n[g] < 4:
            n[g] = 0
            failed[g] = "the chains' common window has fewer than 8 iterations"
            continue
        window[g] = (end - 2 * n[g], end)
    ng = n[ci // c] if ci.size else np.zeros(0, dtype=np.int64)
    parts = []
    for half in (0, 1):
        lo, hi = end - (2 - half) * ng, end - (1 - half) * ng
        wh = np.minimum(iv + w, hi) - np.maximum(iv, lo)
        keep = np.nonzero((wh > 0) & (ng > 0))[0]
        parts.append((keep, np.full(keep.size, half, dtype=np.int64), wh[keep]))
    pos = np.concatenate([p[0] for p in parts])
    half = np.concatenate([p[1] for p in parts])
    wh = np.concatenate([p[2] for p in parts])
    order = np.lexsort((pos, half, ci[pos]))
    pos, half, wh = pos[order], half[order], wh[order]
    key = 2 * ci[pos] + half                                   # ascending: one value per series
    chains = np.unique(ci[pos])
    series_start = np.searchsorted(key, np.repeat(2 * chains, 2) + np.tile([0, 1], chains.size)).astype(np.int64)
    series_start = np.concatenate((series_start, [pos.size])).astype(np.int64)
    group_start = (2 * np.searchsorted(chains // c, np.arange(G + 1))).astype(np.int64)
    return dict(ci=ci[pos], ri=ri[pos], w=wh.astype(np.int64), series_start=series_start, group_start=group_start,
                chains=chains, n=n, window=window, first_iter=first_iter, failed=failed)
