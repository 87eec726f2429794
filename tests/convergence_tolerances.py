"""The one tolerance between bh_autocov_sets (and its host twin) and the numpy restatement (tests/convergence_ref.py).

Both subtract the same mean from the same values with one rounding, so both sum the same m = n - k products of
identically rounded y_t.  They differ in how:

    the library     acc = fma(y_t, y_{t+k}, acc) for ascending t: the products are not rounded, the m additions are;
    the restatement np.dot: every product rounded once, then summed in numpy's own (blocked, pairwise) order;

and both divide by n once.  A sum of m terms in ANY order is within (m - 1) u sum|p_t| of the exact sum to first order
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), u = 2^-53; numpy's rounded products add u sum|p_t|,
the two divisions 2 u |result| <= 2 u sum|p_t|.  So

    |acov_lib - acov_numpy| <= (n - k + 2) 2^-53 sum_t |y_t y_{t+k}| / n.

Nothing looser is used anywhere, and no number here comes from a run.  A NaN must be a NaN on both sides, and a lag
k >= n exactly 0."""
import numpy as np

U = 2.0 ** -53


def acov_bound(n, nlags, absprod):
    """The bound per lag for a series of n samples: absprod [.., nlags] = sum_t |y_t y_{t+k}| / n."""
    k = np.arange(nlags)
    return np.maximum(n - k + 2, 0) * U * np.asarray(absprod)


def check_acov(got, want, length, absprod, what=''):
    """got, want, absprod [series, columns, nlags], length [series]."""
    worst = 0.
    for s, n in enumerate(length):
        tol = acov_bound(int(n), got.shape[2], absprod[s])
        nan = np.isnan(want[s])
        assert np.array_equal(np.isnan(got[s]), nan), (what, s)
        assert np.all(got[s][:, int(n):] == 0), (what, s)
        d = np.abs(got[s] - want[s])
        ok = nan | (d <= tol)
        assert ok.all(), (what, s, int(n), np.argwhere(~ok)[:3], d[~ok][:3], tol[~ok][:3])
        with np.errstate(invalid='ignore', divide='ignore'):
            r = np.where(tol > 0, d / tol, 0.)
        worst = max(worst, np.nanmax(r) if r.size else 0.)
    return worst


def input_bounds(mean, absprod, n):
    """What separates the library's inputs of the rules from the restatement's, per series: its mean by an any-order
    summation error of its n values, (n + 1) u mean|x_t|, bounded here through sqrt(absprod[0]) = rms(y):
    |x_t| <= |mean| + |y_t|, so |dm| <= (n + 1) u (|mean| + rms y); and each autocovariance by acov_bound plus what a
    mean off by dm moves it: sum_t (y_t + y_{t+k}) dm / n + dm^2, at most 2 |dm| rms(y) + dm^2 (Cauchy-Schwarz).
    mean [M], absprod [M, K] -> (dm [M], da [M, K])."""
    mean, absprod = np.asarray(mean, dtype=np.float64), np.asarray(absprod, dtype=np.float64)
    rms = np.sqrt(absprod[:, 0])
    dm = (n + 1) * U * (np.abs(mean) + rms)
    da = acov_bound(n, absprod.shape[1], absprod) + (2 * dm * rms + dm * dm)[:, None]
    return dm, da


def propagate(f, mean, acov, dm, da, keys):
    """First-order worst case of f(mean, acov)[key] under |mean - mean'| <= dm, |acov - acov'| <= da: sum_i |df/dx_i|
    bound_i, the derivatives by forward differences of relative step 2^-20 (their own error, 2^-33 of the term, and the
    second order are covered by the factor 1.01), plus 32 u |f| for the roundings of evaluating f twice.
    -> {key: tolerance}.  The rules are smooth in their inputs as long as Geyer's cut stays where it is; f must return
    'cut', and a step that moves it is an assertion."""
    mean, acov = np.asarray(mean, dtype=np.float64), np.asarray(acov, dtype=np.float64)
    base = f(mean, acov)
    tol = {k: 0. for k in keys}
    for arr, bound in ((mean, dm), (acov, da)):
        flat, b = arr.reshape(-1), np.asarray(bound).reshape(-1)
        for i in range(flat.size):
            if b[i] == 0:
                continue
            h = max(abs(flat[i]), b[i] * 2. ** 20) * 2. ** -20
            x = flat.copy()
            x[i] += h
            moved = f(*( (x.reshape(arr.shape), acov) if arr is mean else (mean, x.reshape(arr.shape)) ))
            assert moved['cut'] == base['cut']
            for k in keys:
                tol[k] += abs(moved[k] - base[k]) / h * b[i]
    return {k: 1.01 * tol[k] + 32 * U * abs(base[k]) for k in keys}
