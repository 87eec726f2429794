"""Tolerances of the velocity-depth posterior (bayhunter_amd/posterior.py) against the reference.

Every value on the depth grid is one of the stored Vs values exactly (the interface depths are the
reference's own sequential fp64 cumsum and the layer lookup is a comparison), so the order statistics and
every count are compared bit for bit: median, min, max, mode, the histograms, the layer counts, the
least-misfit model.  Only the floating sums differ in their order: the device adds per-block partial sums
in a fixed tree and the blocks in a fixed order, numpy adds row after row.

  mean  Σ w·v / W      relative error of a sum of N positive terms in any order <= (N - 1) eps
                       ~ 1e-16 * N; for the test sizes (<= 3e6 rows) a few 1e-13: 1e-12 relative
  std   sqrt(Σ w·(v - mean)² / W)   two-pass, so no cancellation of large squares; the deviation of the
                       mean enters only at second order, but where all values at a depth are equal std is
                       ~0 and only an absolute bound means anything: 1e-9 relative or 1e-12 absolute
"""
MEAN_RTOL = 1e-12
STD_RTOL = 1e-9
STD_ATOL = 1e-12
