"""Tolerances of the modelled-data statistics (bayhunter_amd/datafits.py, csrc/datafits.hip) against the numpy
restatement (tests/datafits_ref.py) on the same modelled data.

Order statistics, min, max, the median (mean of the two middle order statistics, as np.median), the
histograms and the weighted counts are exact: they are values of the column or integer sums.  Only the
floating sums differ in order (per-block partials in a fixed tree, blocks in a fixed order; numpy row after
row), and the percentiles in how the interpolation is rounded.

  mean  Σ w·y / W    the error of a sum of N terms in any order is <= (N - 1) eps Σ|w·y|; RF columns change
                     sign, so the bound is on Σ w|y| / W, not on |mean|: N ~ 1e6 rows -> ~1e-10 worst case,
                     ~sqrt(N) eps = 1e-13 in practice: 1e-12 · Σ w|y| / W
  std   two-pass, as the velocity-depth posterior: posterior_tolerances.STD_RTOL / STD_ATOL
  percentile  numpy's 'linear' lerp between the order statistics k and k + 1 with the same weight t; the
                     host evaluates the same expression on the same two values: at most a rounding apart
                     in t·(b - a) and the sum, 2 ulp of the larger of |a|, |b|
"""
import numpy as np

from posterior_tolerances import STD_ATOL, STD_RTOL  # noqa: F401 (re-exported)

MEAN_ABS = 1e-12             # times Σ w|y| / W
PCT_ULP = 2


def check_mean(got, y, w):
    w = np.asarray(w, dtype=np.float64)[:, None]
    want = (w * y).sum(axis=0) / w.sum()
    bound = MEAN_ABS * (w * np.abs(y)).sum(axis=0) / w.sum()
    assert np.all(np.abs(got - want) <= bound), np.max(np.abs(got - want) / np.maximum(bound, 1e-300))


def check_percentile(got, want, lo, hi):
    ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
    assert np.all(np.abs(got - want) <= PCT_ULP * ulp), np.max(np.abs(got - want) / ulp)
