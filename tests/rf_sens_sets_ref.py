"""The depth-binned receiver-function sensitivity statistics restated in numpy.longdouble on the expanded matrix (every
row repeated `weight` times), from the definitions in include/bayhunter_amd.h (bh_rf_sens_sets_*): vs_total, to_depth and
the weighted moments as tests/sens_sets_ref.py states them for one row, with a trace's selected samples where that file
has periods, and a row that counts for all samples or for none.
"""
import numpy as np

from sens_sets_ref import KINDS, LD, row_cells  # noqa: F401


def summarize(nlay, h, q, K, rf, w, samples, edges, kind, drho_dvp=0.32):
    """One set: K [R, nout, 4, Lmax], rf [R, >= 1], samples the selected indices (None: all) -> dict(total, excluded, n
    (int; n: the rows that count), mean, var, absmean, sqmean, min, max [nsel, nb + 1] (longdouble; NaN for a set without
    weight)).  absmean = sum w a / W and sqmean = sum w a^2 / W, where a >= |x| is the cell formed from the magnitudes
    of K: the sum of the magnitudes of the terms that make x, which the rounding errors of x scale with when the layers'
    values differ in sign."""
    nlay = np.asarray(nlay)
    w = np.ones(len(nlay), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    samples = np.arange(K.shape[1]) if samples is None else np.asarray(samples)
    Ks = K[:, samples]
    x, model = row_cells(nlay, h, q, Ks, None, edges, kind, drho_dvp)
    a, _ = row_cells(nlay, h, q, np.abs(Ks), None, edges, kind, drho_dvp)
    counts = (w > 0) & model & ~np.isnan(rf[:, 0])
    rows = np.nonzero(counts)[0]
    out = dict(total=int(w[rows].sum()), excluded=int(w[(w > 0) & ~counts].sum()), n=int(rows.size))
    X = np.repeat(x[rows], w[rows], axis=0)                                      # the expanded matrix [W, nsel, cells]
    for k in ('mean', 'var', 'absmean', 'sqmean', 'min', 'max'):
        out[k] = np.full((samples.size, len(edges)), np.nan, dtype=LD)
    if X.shape[0]:
        W = LD(X.shape[0])
        out['mean'] = X.sum(axis=0) / W
        out['var'] = (X * X).sum(axis=0) / W - out['mean'] ** 2
        A = np.repeat(a[rows], w[rows], axis=0)
        out['absmean'], out['sqmean'] = A.sum(axis=0) / W, (A * A).sum(axis=0) / W
        out['min'], out['max'] = X.min(axis=0), X.max(axis=0)
    return out
