"""Derived bounds of the depth-binned sensitivity statistics (csrc/sens_sets_core.h) against the longdouble restatement
(tests/sens_sets_ref.py), computed from the restatement's own sums.  u = 2^-53, n the rows of the set that count for the
period, L the layers of the deepest row (Lmax).

A cell x of one row is a chain of at most L - 1 fma's over terms (d / h) G: one rounding for the overlap d, one for the
quotient, one per fma, and two for a fused G (BH_SENS_KIND_VS_TOTAL): relative error (L + 4) u to first order, on terms
of one sign.  s1 = sum w x is a chain of n fma's in blocks plus the fold, at most n roundings, and the mean one division:

    |mean - ref| <= 2 (n + L + 4) u  sum(w |x|) / W

s2 = sum (w x) x carries the cell's error twice and one more rounding per row for w x; the variance s2 / W - mean^2 adds
the mean's error twice, 2 |mean| |d mean| <= 2 (n + L + 4) u mean^2-ish <= that times sum(w x^2) / W by Cauchy-Schwarz;
together, with the final subtraction and division,

    |var - ref| <= 2 (n + 2 L + 8) u  sum(w x^2) / W

(the factor 2 in front is the slack for second-order terms and for the reference's own longdouble rounding, u 2^-11
relative per operation).
"""
import numpy as np

U = 2.0 ** -53


def mean_bound(n, L, absmean):
    """n [nper] rows that count, absmean [nper, cells] = sum(w |x|) / W of the restatement."""
    return 2.0 * (np.asarray(n, dtype=np.float64)[:, None] + L + 4) * U * np.asarray(absmean, dtype=np.float64)


def var_bound(n, L, sqmean):
    """sqmean [nper, cells] = sum(w x^2) / W of the restatement."""
    return 2.0 * (np.asarray(n, dtype=np.float64)[:, None] + 2 * L + 8) * U * np.asarray(sqmean, dtype=np.float64)
