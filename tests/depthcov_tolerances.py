"""The one tolerance between bh_depthcov_sets (and its host twin) and the numpy restatement (tests/depthcov_ref.py).

Both subtract the same centre from the same values with one float64 rounding, so both sum over the same N rows of a set
the terms w_r d_ri d_rj of identically rounded d.  The library rounds e = w d once, then accumulates the N products e d
in some order of fused or unfused steps -- four rows per MFMA, or one fma per row in the twin -- and adds the block
partials.  The restatement sums in long double.  For a sum of N products accumulated in ANY order, each factor pair
carrying at most one extra rounding and the block addition one more, the standard result (Higham, Accuracy and Stability
of Numerical Algorithms, sections 3.1 and 4.2: every term is multiplied by at most N + 2 factors (1 + delta), |delta| <=
u) is

    |S^_ij - S_ij| <= gamma_{N+2} sum_r w_r |d_ri| |d_rj|,     gamma_m = m u / (1 - m u),  u = 2^-53,

and the same for r1 with sum_r w_r |d_ri|.  (A chain of N additions has N - 1 roundings and a product in an fma none;
N + 2 covers every order, with the rounding of w d and of the block addition.)  The right-hand sums are the
restatement's, in long double.  The bound is asserted per cell: a cell whose terms cancel to ~0 is held to the size of
its terms, not to a relative error.  `total` is an integer and exact.

cov = (S - r1 r1^T / W) / W on the host adds, to first order in the inputs' errors dS, dr,

    |dcov_ij| <= (dS_ij + (|r1_i| dr_j + |r1_j| dr_i + dr_i dr_j) / W) / W + 4 u (|S_ij| + |r1_i r1_j| / W) / W,

the last term for the four float64 roundings of the formula itself (product, quotient, difference, quotient), each
relative to a quantity no larger than |S_ij| + |r1_i r1_j| / W.  Two centres give two sets of rounded d; against the
moments of the unrounded x - c each factor is off by one more u, (1 + u)^2 - 1 <= 3 u on the products (`recentred`).
No number here comes from a run."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1. - m * U)


def moment_bounds(ref, z, recentred=False):
    """(bound on S [K, K], bound on r1 [K]) of set z of depthcov_ref.moments' dict."""
    g = gamma(ref['terms'][z] + 2)
    extra = 3 * U if recentred else 0.
    return (g + extra) * ref['absS'][z], (g + extra) * ref['absr1'][z]


def check_moments(S, r1, total, ref, what=''):
    """Every cell of S and r1 of every set within the bound, total exact, nothing where the restatement has nothing
    -> the worst |difference| / bound."""
    worst = 0.
    assert np.array_equal(np.asarray(total), ref['total']), (what, total, ref['total'])
    for z in range(len(ref['total'])):
        bS, b1 = moment_bounds(ref, z)
        dS, d1 = np.abs(np.asarray(S[z], dtype=LD) - ref['S'][z]), np.abs(np.asarray(r1[z], dtype=LD) - ref['r1'][z])
        assert np.all(dS <= bS), (what, z, np.argwhere(dS > bS)[:3], dS[dS > bS][:3], bS[dS > bS][:3])
        assert np.all(d1 <= b1), (what, z, np.argwhere(d1 > b1)[:3], d1[d1 > b1][:3], b1[d1 > b1][:3])
        if ref['total'][z] == 0:
            assert not np.any(S[z]) and not np.any(r1[z]), (what, z)
        with np.errstate(invalid='ignore', divide='ignore'):
            for d, b in ((dS, bS), (d1, b1)):
                r = np.where(b > 0, d / b, 0.)
                worst = max(worst, float(r.max()) if r.size else 0.)
    return worst


def cov_bound(ref, z, recentred=False):
    """The bound on cov [K, K] of set z from the bounds of its moments (module docstring)."""
    bS, b1 = moment_bounds(ref, z, recentred)
    W = LD(ref['total'][z])
    r1, S = np.abs(ref['r1'][z]), np.abs(ref['S'][z])
    cross = np.outer(r1, b1) + np.outer(b1, r1) + np.outer(b1, b1)
    return (bS + cross / W) / W + 4 * U * (S + np.outer(r1, r1) / W) / W
