"""Plain numpy restatement of the convergence diagnostics (bayhunter_amd/convergence.py, csrc/autocov.hip): rows are
expanded with np.repeat, the autocovariances are direct dot products with the mean handed in, and the published formulas
(Gelman et al., BDA3 section 11.4; Vehtari et al. 2021 without rank normalisation) do the rest.  Nothing here is shared
with the code under test."""
import numpy as np


def expand(D, weights, a, b):
    """Rows a:b of D, each repeated `weight` times."""
    D = np.asarray(D, dtype=np.float64)
    if weights is None:
        return D[a:b].copy()
    return np.repeat(D[a:b], np.asarray(weights, dtype=np.int64)[a:b], axis=0)


def autocov(D, weights, series_start, mean, nlags, ncols=None):
    """What bh_autocov_sets returns: per series and column sum_t y_t y_{t+k} / n for k < nlags, y = x - mean; 0 for
    k >= n -> (acov [series, ncols, nlags], length [series], absprod [series, ncols, nlags] = sum_t |y_t y_{t+k}| / n,
    what the tolerance scales with)."""
    D = np.asarray(D, dtype=np.float64)
    K = D.shape[1] if ncols is None else ncols
    S = len(series_start) - 1
    acov, absprod = np.zeros((S, K, nlags)), np.zeros((S, K, nlags))
    length = np.zeros(S, dtype=np.int64)
    for s in range(S):
        x = expand(D, weights, int(series_start[s]), int(series_start[s + 1]))[:, :K]
        n = length[s] = x.shape[0]
        for c in range(K):
            y = x[:, c] - mean[s][c]
            for k in range(min(nlags, n)):
                acov[s, c, k] = np.dot(y[:n - k], y[k:]) / n
                absprod[s, c, k] = np.dot(np.abs(y[:n - k]), np.abs(y[k:])) / n
    return acov, length, absprod


def diagnose(mean, acov, n):
    """Split R-hat, tau and ESS of one column from M series of length n (mean [M], acov [M, K], acov divided by n)."""
    mean, acov = np.asarray(mean, dtype=np.float64), np.asarray(acov, dtype=np.float64)
    M, K = acov.shape
    var = acov * n / (n - 1.)
    W = var[:, 0].mean()
    B = n * mean.var(ddof=1)
    var_plus = (n - 1.) / n * W + B / n
    out = dict(W=W, B=B, var_plus=var_plus, mean=mean.mean(), constant=bool(W == 0), rhat=np.nan, tau=np.nan, ess=np.nan,
               truncated=False, cut=None)
    if not W > 0:
        return out
    out['rhat'] = np.sqrt(var_plus / W)
    T = min(K, n)
    rho = 1. - (W - var[:, :T].mean(axis=0)) / var_plus
    pairs = [rho[2 * k] + rho[2 * k + 1] for k in range(T // 2)]
    cut = next((k for k, p in enumerate(pairs) if p < 0), None)
    out['cut'] = cut
    out['truncated'] = cut is None
    kept = pairs if cut is None else pairs[:cut]
    if not kept:
        return out
    out['tau'] = -1. + 2. * np.sum(np.minimum.accumulate(kept))
    out['ess'] = M * n / out['tau']
    out['rho'] = rho[:2 * len(kept)]
    return out


def ar1_set(rs, phi, entries, wmax, window=None, chains=4, scale=1., shift=0.):
    """`chains` chains of an AR(1) process with coefficient phi, run-length coded: `entries` values per chain, each
    held for 1 .. wmax iterations; the last `window` iterations (default: what the shortest chain has) cut into two
    halves as selection.half_chain_series cuts them -> (D [rows, 1], w [rows], series_start [2 chains + 1], n)."""
    vals, wts = [], []
    for _ in range(chains):
        e = rs.randn(entries)
        x = np.empty(entries)
        x[0] = e[0] / np.sqrt(1. - phi * phi) if phi else e[0]
        for i in range(1, entries):
            x[i] = phi * x[i - 1] + e[i]
        vals.append(x * scale + shift)
        wts.append(rs.randint(1, wmax + 1, entries).astype(np.int64))
    total = min(int(w.sum()) for w in wts)
    n = (total if window is None else int(window)) // 2
    assert 2 * n <= total
    D, W, start = [], [], [0]
    for x, w in zip(vals, wts):
        end = int(w.sum())
        at = np.concatenate(([0], np.cumsum(w)))                    # entry i spans [at[i], at[i + 1])
        for lo, hi in ((end - 2 * n, end - n), (end - n, end)):
            part = np.minimum(at[1:], hi) - np.maximum(at[:-1], lo)
            keep = part > 0
            D.append(x[keep])
            W.append(part[keep])
            start.append(start[-1] + int(keep.sum()))
    return np.concatenate(D)[:, None], np.concatenate(W).astype(np.int32), np.asarray(start, dtype=np.int64), n


def ar1_sets():
    """The four sets of the rules' tests: (name, D, w, series_start, n, nlags).  Each has an outcome that follows from
    the process (tests/test_convergence.py says how): three whose autocorrelation reaches its noise long before the
    last lag, one that is cut off at 16 lags while it still stands at 0.66."""
    rs = np.random.RandomState(5)
    out = []
    for name, phi, entries, wmax, window, nlags in (('phi 0.8', 0.8, 1500, 4, 1200, 512), ('phi 0.5', 0.5, 2000, 1, None, 64),
                                                    ('white', 0., 500, 1, 400, 128), ('phi 0.95 short', 0.95, 600, 3, None, 16)):
        out.append((name,) + ar1_set(rs, phi, entries, wmax, window) + (nlags,))
    return out


def same(a, b):
    """Equal bit for bit, NaN equal to NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def series_case(T, nlags, ncols=5, seed=11, weighted=True):
    """The kernel tests' series around a tile of T samples: expanded lengths 0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1,
    T + nlags + 1, 3 T + 7, and one row of weight 3 T + 5; weights 0 .. 5 with zeros (every series still reaches its
    length exactly); the columns differ in scale and offset, one of them constant
    -> (D [rows, ncols], w int32 [rows] or None, series_start, lengths)."""
    rs = np.random.RandomState(seed)
    lengths = [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, T + nlags + 1, 3 * T + 7]
    rows, wts, start = [], [], [0]
    for n in lengths:
        if weighted:
            w = []
            while sum(w) < n:
                w.append(min(int(rs.randint(0, 6)), n - sum(w)))
            w += [0] * int(rs.randint(0, 3))                       # absent rows at a series' end too
        else:
            w = [1] * n
        wts += w
        start.append(start[-1] + len(w))
    if weighted:
        wts.append(3 * T + 5)
        start.append(start[-1] + 1)
        lengths = lengths + [3 * T + 5]
    R = len(wts)
    D = rs.randn(R, ncols) * np.array([1., 30., 1e-3, 5., 0.][:ncols]) + np.array([0., -200., 0.01, 1e4, 3.5][:ncols])
    w = np.asarray(wts, dtype=np.int32) if weighted else None
    if weighted:
        assert (w == 0).mean() >= 0.1
    return D, w, np.asarray(start, dtype=np.int64), np.asarray(lengths, dtype=np.int64)


def series_means(D, w, start):
    """np.mean of every series' expanded columns (0 for an empty series)."""
    out = np.zeros((len(start) - 1, D.shape[1]))
    for s in range(len(start) - 1):
        x = expand(D, w, int(start[s]), int(start[s + 1]))
        if x.shape[0]:
            out[s] = x.mean(axis=0)
    return out
