"""Derived bounds of the depth-binned receiver-function sensitivity statistics (csrc/rf_sens_sets_core.h on top of
csrc/sens_sets_core.h) against the longdouble restatement (tests/rf_sens_sets_ref.py), computed from the restatement's own
sums.  u = 2^-53, n the rows of the set that count, L the layers of the deepest row (Lmax).

The register blocking changes which thread forms a cell, not how: per (sample, cell) the operations are sens_sets_cell's
in its order, and the sums are sens_sets_core.h's.  The derivation follows tests/sens_sets_tolerances.py, with one
difference.  That file takes the terms (d / h) G of a cell to be of one sign and scales the cell's error with |x|.  A
receiver-function kernel changes sign from layer to layer, and a bin that spans several layers then holds a cell far
smaller than its terms.  So the errors are scaled with

    a = the cell formed from the magnitudes of K (for 'vs_total': |K_vs| + q (|K_vp| + drho_dvp |K_rho|)) >= |x|,

the sum of the magnitudes of everything that is added up to x.  With A1 = sum(w a) / W and A2 = sum(w a^2) / W:

A cell is a chain of at most L - 1 fma's over terms (d / h) G: one rounding for the overlap d, one for the quotient, one
per fma, two for a fused G: |dx| <= (L + 4) u a to first order.  s1 = sum w x is a chain of n fma's in blocks plus the
fold, at most n roundings of partial sums none of which exceeds sum(w a), and the mean one division:

    |mean - ref| <= 2 (n + L + 4) u  A1

s2 = sum (w x) x carries the cell's error twice, 2 (L + 4) u w a^2 a row, one more rounding per row for w x and the
chain's n roundings: (n + 2 L + 9) u A2 W.  The variance s2 / W - mean^2 adds the mean's error twice, 2 |mean| |d mean|
<= 2 (n + L + 4) u A1^2 <= 2 (n + L + 4) u A2 by Cauchy-Schwarz, and two roundings of its own:

    |var - ref| <= 2 (3 n + 4 L + 19) u  A2

(the factor 2 in front is the slack for second-order terms and for the reference's own longdouble rounding, u 2^-11
relative per operation).

tests/test_gpu_pool_rf_sensitivity.py holds ChainPool.rf_sensitivity to the same two bounds against the numpy restatement
in float64 (sensitivity.rf_batch + vs_total + to_depth, summed in longdouble), as tests/test_gpu_pool_sensitivity.py does
for the dispersion kernels: that reference rounds its cells too (vs_total unfused, to_depth's matrix product), by no more
than the (L + 4) u a the bound allows a cell, which the factor 2 covers.

Worst error over bound as measured (what the tests printed; they assert the bounds, not these figures):
    WORST_TWIN   the host twin against the restatement, tests/test_rf_sens_sets.py on x86-64 with fma
    WORST_POOL   ChainPool.rf_sensitivity against the pool-level restatement on one MI355X
"""
import numpy as np

from sens_sets_tolerances import U

WORST_TWIN = {'mean': 0.0811, 'var': 0.0333}
WORST_POOL = {'mean': 0.0493, 'var': 0.0191}


def mean_bound(n, L, absmean):
    """n rows that count, absmean [nsel, cells] = A1 of the restatement."""
    return 2.0 * (float(n) + L + 4) * U * np.asarray(absmean, dtype=np.float64)


def var_bound(n, L, sqmean):
    """sqmean [nsel, cells] = A2 of the restatement."""
    return 2.0 * (3 * float(n) + 4 * L + 19) * U * np.asarray(sqmean, dtype=np.float64)
