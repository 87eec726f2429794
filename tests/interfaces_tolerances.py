"""Tolerances of the jump moments of the discontinuity statistics (bayhunter_amd/interfaces.py) against the
longdouble restatement (tests/interfaces_ref.py).

Every count is an integer sum and every depth and jump is formed by the same float64 expressions as in the
restatement, so all integer fields are compared exactly.  Only the two float sums of a depth bin differ: the device
(and its host twin) adds the N terms of the bin -- one per interface of a row of positive weight, NOT expanded by the
weights -- in its own fixed order through per-wave and per-block partials, the restatement adds the expanded jumps in
longdouble (its own error, ~2^-64 per addend, is neglected against 2^-53).  With u = 2^-53:

  jump_mean = fl(S^ / C),  S^ the computed sum of the terms a_i = fl(w_i J_i), C the integer count of the bin.
      Each a_i carries a relative error <= u, and a sum of N terms in ANY order -- the partials only add levels, at
      most N - 1 additions lie on a term's path -- is off by at most (N - 1) u sum|a_i| to first order.  Together
      |S^ - S| <= N u A (1 + O(N u)) with A = sum w_i |J_i|, and the division adds u |mean|:

          |jump_mean - mean| <= (1 + SLACK) (N u A / C + u |mean|)                                 =: bm

  jump_std = fl(sqrt(fl(Q^ / C))),  Q^ the computed sum of fl(w_i fl(e_i e_i)), e_i = fl(J_i - m^) with the COMPUTED
      mean m^, |m^ - mean| <= bm.  Exactly, sum w (J - m^)^2 = Q + C (m^ - mean)^2 (Q about the true mean).  A term
      carries 4 u (the subtraction twice through the square, the square, the product), the sum N u as above, the
      division and the root u each, so with V = Q / C the true variance

          |V^ - V| <= bm^2 + (N + 6) u (V + bm^2)                                                  =: E
          |jump_std - std| <= (1 + SLACK) (min(sqrt(E), E / std) + u std)

      (|a - b| <= sqrt|a^2 - b^2| for a, b >= 0 covers a bin whose jumps are all equal, std = 0; E / std is the
      first-order form elsewhere).

SLACK = 0.01 stands for the terms of second order in N u (N <= 1e7 here: N u <= 1e-9).  Nothing in the bounds comes
from the code under test.

Worst error seen, as a fraction of the bound: host twin (tests/test_interfaces.py, the random campaign of 4 000 rows
in 12 depth bins, both dtypes) jump_mean 1.1e-4, jump_std 9.3e-4 -- bins of thousands of addends, where the worst case
of N u is far from what rounding errors of both signs add up to; device (tests/test_gpu_interfaces.py, sets of 1 to
3 000 rows, both dtypes) jump_mean 0.0098 and jump_std 0.096 over 20 depth bins, jump_mean 0.63 and jump_std 0.62 over
400 depth bins, where a bin of one or two addends leaves the bound at about one rounding.
"""
import numpy as np

U = 2.0 ** -53
SLACK = 0.01


def mean_bound(addends, absum, count, mean):
    """bm per depth bin (float64 arrays; NaN where count is 0)."""
    addends, absum, count = (np.asarray(x, dtype=np.float64) for x in (addends, absum, count))
    with np.errstate(invalid='ignore', divide='ignore'):
        return (1. + SLACK) * (addends * U * absum / count + U * np.abs(np.asarray(mean, dtype=np.float64)))


def std_bound(addends, absum, count, mean, std):
    bm = mean_bound(addends, absum, count, mean)
    std = np.asarray(std, dtype=np.float64)
    var = std * std
    E = bm * bm + (np.asarray(addends, dtype=np.float64) + 6.) * U * (var + bm * bm)
    with np.errstate(invalid='ignore', divide='ignore'):
        first = np.where(std > 0, E / std, np.inf)
    return (1. + SLACK) * (np.minimum(np.sqrt(E), first) + U * std)
