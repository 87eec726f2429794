"""Independent reference for the group-velocity sensitivity kernels dU/dm and for dU/dT, in numpy.longdouble.

No Rodi formula and no implicit-function theorem.  The secular functions are sensitivity_ref's (nothing of swd_core.h or
sens_core.h).  For a model -- perturbed or not -- the root is solved again at the period and at four neighbouring ones,

    c_T = Richardson of the central differences of the root over T (1 +- E1) and T (1 +- E2),
    U   = c / (1 + (T / c) c_T),

and the derivative of U with respect to a layer parameter, or to T, is a central difference of THAT U at the relative
steps STEP1 and STEP2 with one Richardson step (4 D2 - D1) / 3; |D2 - D1| is kept as the reference's own error estimate,
as in sensitivity_ref.  The perturbed values are rounded to float64 first and the differences taken between the rounded
values.

Roots: sensitivity_ref's bisection takes 45 evaluations for a bracket of 1e-4; twenty roots per slot make that too slow,
so the bracket (which must show a sign change, as there) is closed by the Illinois form of regula falsi, which keeps the
bracket, until a step is below RTOL = 1e-17 relative -- 8 to 10 evaluations.

Sizes.  E1 = 2^-9, E2 = 2^-10: the Richardson step leaves O(E^4) of c_T, 1e-12 times a fifth derivative of order 10..100,
beside a rounding error of 1e-17 c / E = 1e-14.  STEP1 = 2^-15, STEP2 = 2^-16: U carries about 1e-13 of rounding, which
the difference divides by the step (some 1e-09 of U / m), and |D2 - D1|, the truncation of the wider step that the
Richardson step removes, is of the same size -- measured: a few 1e-09 of max |K| (sens_group_tolerances.REFERENCE_OWN).
"""
import numpy as np

import sensitivity_ref as ref

LD = np.longdouble
RTOL = LD(1e-17)
E1, E2 = 2.0 ** -9, 2.0 ** -10
STEP1, STEP2 = 2.0 ** -15, 2.0 ** -16
KINDS = ref.KINDS


def root(model, period, lo, hi, wave):
    """The root of the secular function in (lo, hi): regula falsi (Illinois) on a bracket with a sign change."""
    f = ref.SECULAR[wave]
    a, b = LD(lo), LD(hi)
    fa, fb = f(*model, period, a), f(*model, period, b)
    if not (np.isfinite(fa) and np.isfinite(fb)) or np.signbit(fa) == np.signbit(fb):
        raise ValueError('no sign change between %r and %r' % (lo, hi))
    x, side = a, 0
    for _ in range(100):
        xn = b - fb * (b - a) / (fb - fa)
        if not (a < xn < b):
            xn = (a + b) / 2
        fx = f(*model, period, xn)
        done = abs(xn - x) <= RTOL * abs(xn) or fx == 0 or b - a <= RTOL * a
        x = xn
        if done:
            break
        if np.signbit(fx) == np.signbit(fb):
            if side == 1:
                fa = fa / 2                           # the end kept twice running counts half: no end stays for ever
            b, fb, side = x, fx, 1
        else:
            if side == -1:
                fb = fb / 2
            a, fa, side = x, fx, -1
    # (a hundred steps without one below RTOL: the secular function's own rounding moves the root by more; the value
    # is inside the bracket, and what the rounding does to a derivative shows in the caller's error estimate)
    return x


def _c(model, period, guess, wave, width):
    return root(model, period, guess * (1 - LD(width)), guess * (1 + LD(width)), wave)


def group_velocity(model, period, cguess, wave, width):
    """(U, c, c_T) of the model at the period; the roots are sought within `width` (relative) of cguess and of its
    tangent."""
    T = np.float64(period)
    c = _c(model, T, cguess, wave, width)
    d = []
    for e in (E1, E2):
        tp, tm = np.float64(T * (1.0 + e)), np.float64(T * (1.0 - e))
        # |T c_T| <= c (the scaling identity of the thicknesses, every term of one sign in these models): +- 2 e c
        cp = _c(model, tp, c, wave, 2 * e)
        cm = _c(model, tm, c, wave, 2 * e)
        d.append((cp - cm) / (LD(tp) - LD(tm)))
    cT = (4 * d[1] - d[0]) / 3
    return c / (1 + (LD(T) / c) * cT), c, cT


def _dU(model, period, cstar, wave, kind, idx, r):
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
        U, _, _ = group_velocity(tuple(m), t, cstar, wave, 4 * r)      # |m dc/dm| <= c, as in sensitivity_ref
        ends.append((LD(x), U))
    return (ends[0][1] - ends[1][1]) / (ends[0][0] - ends[1][0])


def derivative(model, period, cstar, wave, kind, idx=0):
    """(value, own error estimate) of dU/d(entry), or of dU/dT for kind 'T'."""
    d1 = _dU(model, period, cstar, wave, kind, idx, STEP1)
    d2 = _dU(model, period, cstar, wave, kind, idx, STEP2)
    return (4 * d2 - d1) / 3, abs(d2 - d1)


def kernels(h, vp, vs, rho, period, c0, wave, slots=None):
    """Everything for one (model, period): dict with U, c, dU_dT, K [4][n] (0 for the half-space's thickness and, for
    Love waves, for vp) and K_err / dU_dT_err, the reference's own error estimates.  slots: the (kind index, layer)
    pairs to compute, NaN elsewhere; None for all.  longdouble."""
    model = ref.round_model(h, vp, vs, rho)
    n = model[0].size
    U, cstar, _ = group_velocity(model, period, LD(c0), wave, 3e-6)
    if slots is None:
        K, E = np.zeros((4, n), dtype=LD), np.zeros((4, n), dtype=LD)
        slots = [(ki, i) for ki, kind in enumerate(KINDS) if not (wave == 'love' and kind == 'vp')
                 for i in range(n - 1 if kind == 'h' else n)]
    else:
        K, E = np.full((4, n), np.nan, dtype=LD), np.full((4, n), np.nan, dtype=LD)
    for ki, i in slots:
        K[ki, i], E[ki, i] = derivative(model, period, cstar, wave, KINDS[ki], i)
    dT, eT = derivative(model, period, cstar, wave, 'T')
    return dict(U=U, c=cstar, dU_dT=dT, dU_dT_err=eT, K=K, K_err=E)
