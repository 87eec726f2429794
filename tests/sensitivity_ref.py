"""Independent reference for the phase-velocity sensitivity kernels dc/dm and for dc/dT, in numpy.longdouble.

Nothing of bayhunter_amd/csrc/swd_core.h or sens_core.h, and no implicit-function theorem: the root of an independent
secular function is solved again in the perturbed model, and the derivative is a central difference of the ROOT.

Secular functions (both are scaled by positive factors on the way up, which moves no root):

* Rayleigh: the two solutions that decay in the half-space, carried to the free surface as motion-stress 4-vectors
  (ellipticity_ref.surface_pair: Thomson-Haskell propagators by a Taylor series, re-orthonormalised); a surface wave
  exists where a combination of the two has no traction, i.e. where the 2x2 minor of their traction rows vanishes.
* Love: the SH motion-stress vector (l1, l2) = (u_y, mu du_y/dz), z down.  In the half-space l = (1, -mu nu),
  nu^2 = k^2 - omega^2 / beta^2 > 0.  A layer of thickness d is crossed upwards by

      l1' = C l1 - S l2 / mu          C = cosh(nu d), S = sinh(nu d) / nu          (nu^2 > 0)
      l2' = -mu nu^2 S l1 + C l2      C = cos(q d),   S = sin(q d) / q, nu^2 = -q^2 (nu^2 < 0)

  and the surface is free where l2 vanishes.

Root: bisection in c between two velocities of opposite sign, to RTOL = 1e-17 relative (eps(longdouble) = 1.1e-19 on
x86-64).  The unperturbed root is sought in c0 (1 +- 3e-6) around the phase velocity c0 the search returned; a root
of a model with one value moved by the relative step r in root (1 +- 4 r): |m dc/dm| <= c for every parameter, by the
scaling identities the tests check.

Derivative: central differences of the root at the relative steps STEP1 = 2^-17 and STEP2 = 2^-18 (the perturbed
values are rounded to float64 first, and the differences are taken between the rounded values), then one Richardson
step (4 D2 - D1) / 3.  |D2 - D1| is kept as the reference's own error estimate: it bounds the truncation error the
Richardson step removes, and holds the rounding error of the two roots (1e-17 c / r).
"""
import numpy as np

import ellipticity_ref as er

LD = np.longdouble
TWOPI = er.TWOPI
RTOL = LD(1e-17)
STEP1, STEP2 = 2.0 ** -17, 2.0 ** -18
KINDS = ('h', 'vp', 'vs', 'rho')


def rayleigh_secular(h, vp, vs, rho, period, c):
    y1, y2 = er.surface_pair(h, vp, vs, rho, period, c)
    return y1[2] * y2[3] - y1[3] * y2[2]


def love_secular(h, vp, vs, rho, period, c):
    h, vs, rho = (np.asarray(x, dtype=np.float64).astype(LD) for x in (h, vs, rho))
    n = h.size
    om = TWOPI / LD(period)
    k = om / LD(c)
    mu = rho * vs * vs
    nu2 = k * k - (om / vs[n - 1]) ** 2
    if not nu2 > 0:
        raise ValueError("the phase velocity is not below the half-space's velocity")
    l1, l2 = LD(1), -mu[n - 1] * np.sqrt(nu2)
    for i in range(n - 2, -1, -1):
        nu2 = k * k - (om / vs[i]) ** 2
        if nu2 > 0:
            nu = np.sqrt(nu2)
            e1 = np.expm1(-2 * nu * h[i])                  # (1 - e needs it where c has just fallen below this layer's vs)
            C, S = (2 + e1) / 2, -e1 / (2 * nu)            # cosh, sinh / nu, both times exp(-nu d) > 0
        elif nu2 < 0:
            q = np.sqrt(-nu2)
            C, S = np.cos(q * h[i]), np.sin(q * h[i]) / q
        else:
            C, S = LD(1), h[i]
        l1, l2 = C * l1 - S * l2 / mu[i], -mu[i] * nu2 * S * l1 + C * l2
        s = max(abs(l1), abs(l2))
        l1, l2 = l1 / s, l2 / s
    return l2


SECULAR = {'rayleigh': rayleigh_secular, 'love': love_secular}


def root(model, period, lo, hi, wave):
    """The root of the secular function in (lo, hi) by bisection; ValueError when the signs at the ends agree."""
    f = SECULAR[wave]
    lo, hi = LD(lo), LD(hi)
    flo, fhi = f(*model, period, lo), f(*model, period, hi)
    if not (np.isfinite(flo) and np.isfinite(fhi)) or np.signbit(flo) == np.signbit(fhi):
        raise ValueError('no sign change between %r and %r' % (lo, hi))
    while hi - lo > RTOL * lo:
        mid = (lo + hi) / 2
        fm = f(*model, period, mid)
        if np.signbit(fm) == np.signbit(flo):
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def round_model(h, vp, vs, rho):
    """The real*4 layers the library works on, as float64."""
    return tuple(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64) for x in (h, vp, vs, rho))


def base_root(model, period, c0, wave):
    return root(model, period, LD(c0) * (1 - LD(3e-6)), LD(c0) * (1 + LD(3e-6)), wave)


def _droot(model, period, cstar, wave, kind, idx, r):
    """Central difference of the root over entry (kind, idx) of the model, or over the period (kind 'T')."""
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
        c = root(tuple(m), t, cstar * (1 - LD(4 * r)), cstar * (1 + LD(4 * r)), wave)
        ends.append((LD(x), c))
    return (ends[0][1] - ends[1][1]) / (ends[0][0] - ends[1][0])


def derivative(model, period, cstar, wave, kind, idx=0):
    """(value, own error estimate) of dc/d(entry): Richardson on STEP1, STEP2."""
    d1 = _droot(model, period, cstar, wave, kind, idx, STEP1)
    d2 = _droot(model, period, cstar, wave, kind, idx, STEP2)
    return (4 * d2 - d1) / 3, abs(d2 - d1)


def kernels(h, vp, vs, rho, period, c0, wave):
    """Everything for one (model, period): dict with c (the root), dc_dT, K [4][n] (0 for the half-space's thickness
    and, for Love waves, for vp), and K_err / dc_dT_err, the reference's own error estimates.  longdouble."""
    model = round_model(h, vp, vs, rho)
    n = model[0].size
    cstar = base_root(model, period, c0, wave)
    K, E = np.zeros((4, n), dtype=LD), np.zeros((4, n), dtype=LD)
    for ki, kind in enumerate(KINDS):
        if wave == 'love' and kind == 'vp':
            continue
        for i in range(n - 1 if kind == 'h' else n):
            K[ki, i], E[ki, i] = derivative(model, period, cstar, wave, kind, i)
    dT, eT = derivative(model, period, cstar, wave, 'T')
    return dict(c=cstar, dc_dT=dT, dc_dT_err=eT, K=K, K_err=E)


def group_velocity(h, vp, vs, rho, period, c0, wave, eps=2.0 ** -18):
    """U = c / (1 + (T / c) dc/dT) with dc/dT from the roots at T (1 +- eps): what a finite-difference group velocity
    is in the limit, from this file's roots alone."""
    model = round_model(h, vp, vs, rho)
    cstar = base_root(model, period, c0, wave)
    d = _droot(model, period, cstar, wave, 'T', 0, eps)
    return cstar / (1 + (LD(period) / cstar) * d)
