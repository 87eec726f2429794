"""Independent reference for the ellipticity sensitivity kernels dE/dm and for dE/dT, in numpy.longdouble.

No implicit-function theorem, no G_m + G_c dc/dm, nothing of swd_core.h, sens_core.h or ell_sens_core.h.  For a model
with one entry moved (or at a moved period) the root of sensitivity_ref's secular function is solved again with
sensitivity_ref.root, ellipticity_ref.ellipticity is evaluated at THAT root (normal traction eliminated; at a root the
two eliminations agree), and the derivative is a central difference of that E at the relative steps STEP1 and STEP2
with one Richardson step (4 D2 - D1) / 3.  |D2 - D1| is kept as the reference's own error estimate, as in
sensitivity_ref.  The perturbed values are rounded to float64 first and the differences taken between the rounded
values.

Sizes.  The root is known to RTOL = 1e-17 relative and E moves by c G_c, a few units, per unit of relative change of c,
so E carries some 1e-16 of rounding, which the difference divides by the step: 1e-11 of E / m at 2^-17.  The truncation
of the wider step, which the Richardson step removes and |D2 - D1| bounds, is (2^-17)^2 = 6e-11 times a third
logarithmic derivative of order 1 .. 100 (ell_sens_tolerances.REFERENCE_OWN has what was measured).
"""
import numpy as np

import ellipticity_ref as er
import sensitivity_ref as ref

LD = np.longdouble
STEP1, STEP2 = 2.0 ** -17, 2.0 ** -18
KINDS = ref.KINDS


def ellipticity_at_root(model, period, lo, hi):
    """(E, c): the root of the Rayleigh secular function in (lo, hi) and the signed H/V there."""
    c = ref.root(model, period, lo, hi, 'rayleigh')
    r1, r2 = er.surface_motion(*model, period, c, 'tz')
    return -r1 / r2, c


def _dE(model, period, cstar, kind, idx, r):
    ends = []
    for sign in (1.0, -1.0):
        m = [x.copy() for x in model]
        t = np.float64(period)
        if kind == 'T':
            t = np.float64(t * (1.0 + sign * r))
            x = t
        else:
            a = m[KINDS.index(kind)]
            a[idx] = np.float64(a[idx] * (1.0 + sign * r))
            x = a[idx]
        E, _ = ellipticity_at_root(tuple(m), t, cstar * (1 - LD(4 * r)), cstar * (1 + LD(4 * r)))     # |m dc/dm| <= c
        ends.append((LD(x), E))
    return (ends[0][1] - ends[1][1]) / (ends[0][0] - ends[1][0])


def derivative(model, period, cstar, kind, idx=0):
    """(value, own error estimate) of dE/d(entry), or of dE/dT for kind 'T'."""
    d1 = _dE(model, period, cstar, kind, idx, STEP1)
    d2 = _dE(model, period, cstar, kind, idx, STEP2)
    return (4 * d2 - d1) / 3, abs(d2 - d1)


def kernels(h, vp, vs, rho, period, c0, slots=None):
    """Everything for one (model, period): dict with E, c, dE_dT, K [4][n] (0 for the half-space's thickness) and K_err /
    dE_dT_err, the reference's own error estimates.  slots: the (kind index, layer) pairs to compute, NaN elsewhere;
    None for all.  longdouble."""
    model = ref.round_model(h, vp, vs, rho)
    n = model[0].size
    E, cstar = ellipticity_at_root(model, period, LD(c0) * (1 - LD(3e-6)), LD(c0) * (1 + LD(3e-6)))
    if slots is None:
        K, Ke = np.zeros((4, n), dtype=LD), np.zeros((4, n), dtype=LD)
        slots = [(ki, i) for ki, kind in enumerate(KINDS) for i in range(n - 1 if kind == 'h' else n)]
    else:
        K, Ke = np.full((4, n), np.nan, dtype=LD), np.full((4, n), np.nan, dtype=LD)
    for ki, i in slots:
        K[ki, i], Ke[ki, i] = derivative(model, period, cstar, KINDS[ki], i)
    dT, eT = derivative(model, period, cstar, 'T')
    return dict(E=E, c=cstar, dE_dT=dT, dE_dT_err=eT, K=K, K_err=Ke)
