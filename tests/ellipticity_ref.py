"""Independent reference for the Rayleigh-wave ellipticity (H/V) of a layered half-space, in numpy.longdouble.

No compound (Dunkin) matrices and nothing of bayhunter_amd/csrc/ell_core.h: the two solutions that decay in the
half-space are carried up to the free surface as motion-stress 4-vectors by Thomson-Haskell propagators and
re-orthonormalised on the way, and the surface motion is the combination of the two whose traction vanishes.

Conventions (Aki & Richards, Quantitative Seismology, section 7.2; z down, wave towards +x, theta = k x - omega t):

    u_x = r1(z) exp(i theta)        tau_zx = r3(z) exp(i theta)      r3 = mu (r1' - k r2)
    u_z = i r2(z) exp(i theta)      tau_zz = i r4(z) exp(i theta)    r4 = (lambda + 2 mu) r2' + k lambda r1

    d/dz (r1, r2, r3, r4) = A (r1, r2, r3, r4),   zeta = 4 mu (lambda + mu) / (lambda + 2 mu),

        A = [[ 0,                       k,           1 / mu,  0                        ],
             [-k lambda / (lambda+2mu), 0,           0,       1 / (lambda + 2 mu)      ],
             [ k^2 zeta - omega^2 rho,  0,           0,       k lambda / (lambda + 2mu)],
             [ 0,                      -omega^2 rho, -k,      0                        ]]

(the two equations of motion with the two stress definitions solved for the derivatives).  In a homogeneous layer
the propagator over dz is exp(A dz).  The half-space solutions are the P and SV waves that decay with depth,
(r1, r2) = (k, nu_a) exp(-nu_a z) and (nu_b, k) exp(-nu_b z), nu^2 = k^2 - omega^2 / v^2; half_space_vectors()
checks that they are eigenvectors of A.

Sign.  In a homogeneous half-space the surface motion is u_x = 0.42 sin(omega t), u_z = 0.62 cos(omega t) at x = 0
(Poisson solid, z down): at its deepest point the particle moves forward, the motion is retrograde, and in the
convention above r1 and r2 have opposite signs.  H/V is returned as -r1 / r2: positive for retrograde motion,
negative in a prograde window.

Numerics.  The stresses are carried as r3 / (k mu0), r4 / (k mu0) (mu0: the half-space's rigidity), which makes every
entry of A of order k.  A layer is crossed in steps of k dz <= 1, each by a scaled-and-squared Taylor series of
exp(-A dz), with a Gram-Schmidt step on the pair of vectors after each: the pair spans the same plane, and the growing
solution cannot swamp the other one.  eps(longdouble) = 1.1e-19 on x86-64.
"""
import numpy as np

LD = np.longdouble
TWOPI = LD(2.0 * 3.141592653589793)          # the double the library divides by the period


def flatten_rayleigh(h, vp, vs, rho):
    """Earth-flattening transformation of surfdisp96.f:486-553 for Rayleigh waves, on real*4 layers: the running
    depth and the logarithms in fp64, the results rounded to real*4."""
    h, vp, vs, rho = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (h, vp, vs, rho))
    n = h.size
    d = h.astype(np.float64)
    d[n - 1] = 1.0
    ar = 6370.0
    dr = np.cumsum(d)                           # (sequential, like the reference's loop)
    r1 = ar - dr
    r0 = np.concatenate(([ar], r1[:-1]))
    z0, z1 = ar * np.log(ar / r0), ar * np.log(ar / r1)
    tmp = (ar + ar) / (r0 + r1)
    dn = (z1 - z0).astype(np.float32)
    dn[n - 1] = 0.0
    # real*4 ** real*4, correctly rounded: the power in longdouble, rounded once (numpy's float32 power is not)
    scale = np.power(tmp.astype(np.float32).astype(LD), LD(np.float32(-2.275))).astype(np.float32)
    return (dn, (vp.astype(np.float64) * tmp).astype(np.float32), (vs.astype(np.float64) * tmp).astype(np.float32),
            (rho * scale).astype(np.float32))


def _system(k, om, a, b, rho, s):
    mu = rho * b * b
    l2m = rho * a * a
    lam = l2m - 2 * mu
    zeta = 4 * mu * (lam + mu) / l2m
    A = np.zeros((4, 4), dtype=LD)
    A[0, 1] = k;                            A[0, 2] = s / mu
    A[1, 0] = -k * lam / l2m;               A[1, 3] = s / l2m
    A[2, 0] = (k * k * zeta - om * om * rho) / s; A[2, 3] = k * lam / l2m
    A[3, 1] = -om * om * rho / s;           A[3, 2] = -k
    return A, mu, lam, l2m


def half_space_vectors(k, om, a, b, rho, s):
    """The decaying P and SV solutions at the top of the half-space, stresses over s; both checked against A."""
    A, mu, lam, l2m = _system(k, om, a, b, rho, s)
    na = np.sqrt(k * k - (om / a) ** 2)
    nb = np.sqrt(k * k - (om / b) ** 2)
    if not (na > 0 and nb > 0):
        raise ValueError("the phase velocity is not below the half-space's velocities")
    yp = np.array([k, na, -2 * mu * k * na / s, (k * k * lam - l2m * na * na) / s], dtype=LD)
    ys = np.array([nb, k, -mu * (nb * nb + k * k) / s, -2 * mu * k * nb / s], dtype=LD)
    for y, nu in ((yp, na), (ys, nb)):
        res = A.dot(y) + nu * y
        assert np.abs(res).max() <= 64 * np.finfo(LD).eps * k * np.abs(y).max(), (res, y)
    return yp, ys


def _expm(M):
    nrm = float(np.abs(M).sum(axis=1).max())
    sq = max(0, int(np.ceil(np.log2(max(nrm, 1e-300)))) + 3)          # |M| / 2^sq <= 1/8
    X = M / LD(2) ** sq
    E = np.eye(4, dtype=LD)
    term = np.eye(4, dtype=LD)
    for j in range(1, 26):                                            # (1/8)^25 / 25! is far below eps
        term = term.dot(X) / LD(j)
        E = E + term
    for _ in range(sq):
        E = E.dot(E)
    return E


def _orthonormalise(y1, y2):
    y1 = y1 / np.sqrt(y1.dot(y1))
    y2 = y2 - y1.dot(y2) * y1
    return y1, y2 / np.sqrt(y2.dot(y2))


def surface_pair(h, vp, vs, rho, period, c):
    """The two half-space solutions at the free surface (orthonormalised; rows r1, r2, r3 / s, r4 / s)."""
    h, vp, vs, rho = (np.asarray(x, dtype=np.float64).astype(LD) for x in (h, vp, vs, rho))
    n = h.size
    om = TWOPI / LD(period)
    k = om / LD(c)
    s = k * rho[n - 1] * vs[n - 1] ** 2
    y1, y2 = _orthonormalise(*half_space_vectors(k, om, vp[n - 1], vs[n - 1], rho[n - 1], s))
    for i in range(n - 2, -1, -1):
        A = _system(k, om, vp[i], vs[i], rho[i], s)[0]
        nsub = max(1, int(np.ceil(float(k * h[i]))))
        P = _expm(-A * (h[i] / nsub))
        for _ in range(nsub):
            y1, y2 = _orthonormalise(P.dot(y1), P.dot(y2))
    return y1, y2


def surface_motion(h, vp, vs, rho, period, c, eliminate='tz'):
    """(r1, r2) at the surface of the combination whose normal ('tz') or shear ('tr') traction vanishes."""
    y1, y2 = surface_pair(h, vp, vs, rho, period, c)
    j = 3 if eliminate == 'tz' else 2
    return y1[0] * y2[j] - y2[0] * y1[j], y1[1] * y2[j] - y2[1] * y1[j]


def ellipticity(h, vp, vs, rho, periods, c, eliminate='tz', flsph=0):
    """Signed H/V per period at the phase velocities c (positive: retrograde), longdouble.  The layers are taken as
    the real*4 values the library rounds them to; flsph = 1 applies flatten_rayleigh first."""
    h, vp, vs, rho = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (h, vp, vs, rho))
    if flsph:
        h, vp, vs, rho = flatten_rayleigh(h, vp, vs, rho)
    out = np.empty(len(periods), dtype=LD)
    for i, (t, ci) in enumerate(zip(periods, c)):
        r1, r2 = surface_motion(h, vp, vs, rho, t, ci, eliminate)
        out[i] = -r1 / r2
    return out


def vertical_changes_sign(h, vp, vs, rho, period, c, rel=1.0e-6, flsph=0, eliminate='tz'):
    """True when the vertical surface displacement (normal traction eliminated, or the shear traction) has a zero
    within rel * c of c: the ratio has a pole there, and a comparison at a c that is only known to rel is meaningless."""
    h, vp, vs, rho = (np.asarray(x, dtype=np.float64).astype(np.float32) for x in (h, vp, vs, rho))
    if flsph:
        h, vp, vs, rho = flatten_rayleigh(h, vp, vs, rho)
    lo = surface_motion(h, vp, vs, rho, period, c * (1 - rel), eliminate)[1]
    hi = surface_motion(h, vp, vs, rho, period, c * (1 + rel), eliminate)[1]
    return bool(np.signbit(lo) != np.signbit(hi))


def rayleigh_root(vp, vs):
    """c of the homogeneous half-space: the root of (2 - c^2/b^2)^2 = 4 sqrt(1 - c^2/a^2) sqrt(1 - c^2/b^2) in
    (0, b), by bisection in longdouble."""
    a, b = LD(vp), LD(vs)

    def f(c):
        s = (c / b) ** 2
        return (2 - s) ** 2 - 4 * np.sqrt(1 - (c / a) ** 2) * np.sqrt(1 - s)
    lo, hi = LD(0.5) * b, b * (1 - LD(2) ** -40)        # f < 0 at 0.5 b for every Vp/Vs > 1.2, f(b) = 1 > 0
    assert f(lo) < 0 < f(hi)
    for _ in range(200):
        mid = (lo + hi) / 2
        if f(mid) < 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def half_space_hv(vp, vs, c):
    """H/V of the homogeneous half-space at velocity c with the normal traction eliminated: from the potentials
    phi = A exp(-nu_a z), psi = B exp(-nu_b z), tau_zz = 0 gives B, and u_x / u_z at z = 0 is
    s b / ((2 - s) - 2 a b), s = c^2/vs^2, a = sqrt(1 - c^2/vp^2), b = sqrt(1 - s).  At the Rayleigh root it is the
    half-space's ellipticity (0.6812 for Vp/Vs = sqrt 3)."""
    c, vp, vs = LD(c), LD(vp), LD(vs)
    s = (c / vs) ** 2
    a, b = np.sqrt(1 - (c / vp) ** 2), np.sqrt(1 - s)
    return s * b / ((2 - s) - 2 * a * b)
