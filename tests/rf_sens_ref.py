"""TEST ONLY.  Independent reference of the receiver-function sensitivity kernels K[t, kind, layer] = dRF(t)/dm: central
differences of hp_oracle.rf_model_ld -- the numpy.longdouble trace of the oracle's C restatement, which shares no code
with the library -- at two relative steps R and R / 2, extrapolated by Richardson:

    D(r)  = (RF(m with the entry times 1 + r) - RF(m with it times 1 - r)) / (v (1 + r) - v (1 - r))
    K     = (4 D(R / 2) - D(R)) / 3                      (the r^2 term of the truncation error removed)
    own   = |D(R / 2) - D(R)| / 3                        (the r^2 term of D(R / 2): an upper estimate of K's own error)

With R = 2^-14 and a trace rounded at 2^-64 the rounding part of D is about 1e-19 / (2 R v) = 1e-15 of the trace's
scale and the truncation part R^2 = 4e-9 times the third derivative's scale: `own` is a few 1e-9 of max|K| on a
differentiable trace.  Where the trace is NOT differentiable in the entry -- a branch of the algorithm switching between
m (1 - R) and m (1 + R) -- D(R) and D(R / 2) differ by a finite fraction of K instead: entries with
own > FLAG * max|K of the kind and model| are reported (`flagged`) and may be left out of a comparison, at most CAP of
the (model, sample, slot) entries of a case list (rf_sens_cases.py checks its lists against the cap).

The half-space has no thickness (K_h = 0 there) and qp, qs are held fixed (500, 225: rf_model_ld's)."""
import numpy as np

import hp_oracle

R = 2.0 ** -20
FLAG = 1.0e-6          # own error above this fraction of max|K| of the kind and model: not differentiable here
CAP = 0.01             # at most this fraction of a case list's entries may be flagged
KINDS = ('h', 'vp', 'vs', 'rho')


def _trace(m, par):
    return hp_oracle.rf_model_ld(m[0], m[1], m[2], m[3], par['p'], par['gauss'], par['nsamp'], par['fsamp'], par['tshift'],
                                 par['nsv'], par['waveno'], par['nout'])


def _diff(model, kind, i, r, par):
    ld = np.longdouble
    out = []
    for f in (ld(1) + ld(r), ld(1) - ld(r)):
        m = [np.array(x, dtype=ld) for x in model]
        m[kind][i] = m[kind][i] * f
        out.append((_trace(m, par), m[kind][i]))
    return (out[0][0] - out[1][0]) / (out[0][1] - out[1][1])


def kernels(h, vp, vs, rho, par):
    """dict K [nout][4][n] (numpy.longdouble), own (the same shape: the reference's estimate of its own error), rf [nout],
    flagged [nout][4][n] bool.  par: p, gauss, nsamp, fsamp, tshift, nsv (None: the top layer's vs), waveno, nout."""
    ld = np.longdouble
    model = [np.asarray(x, dtype=np.float64) for x in (h, vp, vs, rho)]
    n, nout = model[0].size, par['nout']
    K, own = np.zeros((nout, 4, n), dtype=ld), np.zeros((nout, 4, n), dtype=ld)
    for kind in range(4):
        for i in range(n):
            if (kind == 0 and i == n - 1) or model[kind][i] == 0.0:
                continue
            d1, d2 = _diff(model, kind, i, R, par), _diff(model, kind, i, R / 2, par)
            K[:, kind, i] = (4 * d2 - d1) / 3
            own[:, kind, i] = np.abs(d2 - d1) / 3
    scale = np.abs(K).max(axis=(0, 2))                          # per kind
    flagged = own > FLAG * np.where(scale > 0, scale, 1)[None, :, None]
    return dict(K=K, own=own, rf=_trace([np.array(x, dtype=ld) for x in model], par), flagged=flagged)
