"""The one tolerance between bh_datacov_sets (and its host twin) and the numpy restatement (tests/datacov_ref.py).

The argument is depthcov_tolerances': both sides subtract the same centres from the same values with one float64
rounding each, so both sum over the same N rows of a set the terms w_r dx_rk dy_rj of identically rounded dx, dy.  The
library rounds ex = w dx once, then accumulates the N products ex dy in some order of fused or unfused steps -- four rows
per MFMA, or one fma per row in the twin -- and adds the block partials; the restatement sums in long double.  For a
sum of N products accumulated in ANY order, each factor pair carrying at most one extra rounding and the block addition
one more (Higham, Accuracy and Stability of Numerical Algorithms, sections 3.1 and 4.2),

    |C^_kj - C_kj| <= gamma_{N+2} sum_r w_r |dx_rk| |dy_rj|,     gamma_m = m u / (1 - m u),  u = 2^-53,

and the same for qx, qy (the terms w d^2 are their own absolute values, so the right-hand sum is q itself) and for
r1x, r1y with sum_r w_r |d|.  The right-hand sums are the restatement's, in long double.  The bound is asserted per cell.
`total` and `excluded` are integers and exact.

cov = (C - r1x r1y^T / W) / W on the host adds, to first order in the inputs' errors dC, dx, dy,

    |dcov_kj| <= (dC_kj + (|r1x_k| dy_j + |r1y_j| dx_k + dx_k dy_j) / W) / W + 4 u (|C_kj| + |r1x_k r1y_j| / W) / W,

the last term for the four float64 roundings of the formula itself, each relative to a quantity no larger than
|C_kj| + |r1x_k r1y_j| / W; the variances (q - r1^2 / W) / W are the same formula with both factors alike, and a
standard deviation sqrt(v) stays between the square roots of v -+ dv, to one rounding (`std_bound`).  Two centres give
two sets of rounded d; against the moments of the unrounded differences each factor is off by one more u,
(1 + u)^2 - 1 <= 3 u on the products (`recentred`).
No number here comes from a run."""
import numpy as np

from depthcov_tolerances import LD, U, gamma  # noqa: F401

CELLS = (('C', 'absC'), ('r1x', 'absr1x'), ('r1y', 'absr1y'), ('qx', 'qx'), ('qy', 'qy'))


def moment_bounds(ref, z, recentred=False):
    """{name: bound} of set z of datacov_ref.moments' dict for C, r1x, r1y, qx, qy."""
    g = gamma(ref['terms'][z] + 2) + (3 * U if recentred else 0.)
    return {name: g * np.abs(ref[ab][z]) for name, ab in CELLS}


def check_moments(got, ref, what=''):
    """Every cell of every moment of every set within the bound (`got`: dict C, r1x, r1y, qx, qy, total, excluded), the
    two weights exact, nothing where the restatement has nothing -> the worst |difference| / bound."""
    worst = 0.
    assert np.array_equal(np.asarray(got['total']), ref['total']), (what, got['total'], ref['total'])
    assert np.array_equal(np.asarray(got['excluded']), ref['excluded']), (what, got['excluded'], ref['excluded'])
    for z in range(len(ref['total'])):
        bounds = moment_bounds(ref, z)
        for name, _ in CELLS:
            d, b = np.abs(np.asarray(got[name][z], dtype=LD) - ref[name][z]), bounds[name]
            assert np.all(d <= b), (what, name, z, np.argwhere(d > b)[:3], d[d > b][:3], b[d > b][:3])
            if ref['total'][z] == 0:
                assert not np.any(got[name][z]), (what, name, z)
            with np.errstate(invalid='ignore', divide='ignore'):
                r = np.where(b > 0, d / b, 0.)
            worst = max(worst, float(r.max()) if r.size else 0.)
    return worst


def cov_bound(ref, z, recentred=False):
    """The bound on cov [K, S] of set z from the bounds of its moments (module docstring)."""
    b = moment_bounds(ref, z, recentred)
    W = LD(ref['total'][z])
    rx, ry, C = np.abs(ref['r1x'][z]), np.abs(ref['r1y'][z]), np.abs(ref['C'][z])
    cross = np.outer(rx, b['r1y']) + np.outer(b['r1x'], ry) + np.outer(b['r1x'], b['r1y'])
    return (b['C'] + cross / W) / W + 4 * U * (C + np.outer(rx, ry) / W) / W


def var_bounds(ref, z, recentred=False):
    """The bounds on the variances (of the K model columns, of the S data columns) of set z."""
    b = moment_bounds(ref, z, recentred)
    W = LD(ref['total'][z])
    out = []
    for q, r in (('qx', 'r1x'), ('qy', 'r1y')):
        r1 = np.abs(ref[r][z])
        out.append((b[q] + (2 * r1 * b[r] + b[r] ** 2) / W) / W + 4 * U * (ref[q][z] + r1 ** 2 / W) / W)
    return out


def std_bound(var, dvar):
    """The bound on sqrt(v) of a variance v > 0 known to dvar: sqrt is monotone and correctly rounded."""
    var, dvar = np.asarray(var, dtype=LD), np.asarray(dvar, dtype=LD)
    s = np.sqrt(var)
    return np.maximum(np.sqrt(var + dvar) - s, s - np.sqrt(np.maximum(var - dvar, 0))) + U * np.sqrt(var + dvar)
