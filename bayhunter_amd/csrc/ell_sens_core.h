// ell_sens_core.h -- depth sensitivity kernels d(H/V)/dm of the fundamental Rayleigh mode's ellipticity.
//
// ell_core.h: carried to the free surface, Dunkin's vector e gives the period equation F = e[0] and, as a quotient of
// two of its components, the horizontal-to-vertical ratio of the surface motion,
//
//     G(c, T, m) = e[3] / (wvno e[2])   (ELL_FORM_TZ)        -wvno e[2] / e[1]   (ELL_FORM_TR)
//
// at any c.  The ellipticity is G on the dispersion curve, E(T, m) = G(c*(T, m), T, m) with F(c*, T, m) = 0, so
//
//     dE/dm_j = G_mj + G_c dc/dm_j        dc/dm_j = -F_mj / F_c
//     dE/dT   = G_T  + G_c dc/dT          dc/dT   = -F_T  / F_c
//
// with every partial derivative a central difference, as in sens_core.h.  One pass of the recursion (ell_sens_FG)
// yields e[0], e[2] and e[3] together: F and G at once, and every pass sens_root and sens_slot run for dc/dm returns
// the G the ellipticity kernel needs.  G is a quotient of components of the same vector, so swd_dunkin_apply's
// normalisation cancels exactly, off the root too.  Only the total derivative has a meaning: the two forms differ off
// the root (their G_m and G_c differ) and agree along it (tests/test_ell_sens.py compares the two totals).
//
// The pass reads the accessor as doubles.  ell_core.h's pass goes through EllLayer, four floats, which would round a
// value perturbed by 2^-20 back to where it was.
//
// The root is polished as sens_root polishes it, with sens_core.h's own functions: c, F_c, dc/dT and K^c are, bit for
// bit, what the phase pass computes.  E is G at that root in double precision -- not the value ell_kernel returns at
// the stored real*4 c, from which it differs by G_c (c - c0).
//
// Passes per (model, period): the Newton steps of sens_root, 2 for the differences over c, 2 for those over T, 1 for E
// at the polished root; 2 per slot.  The phase pass runs one fewer (it has no use for a pass at the root itself).
//
// No value -- every output of the (model, period) NaN: where sens_root has none (the search's flag, fewer than two
// layers, water on top -- which is also where ell_eval has none --, a stored c that is no positive finite number, a
// polished root outside the accept window, F_c zero or NaN); e[2] zero at the root (no vertical motion: the ratio has
// a pole); E, G_c, F_c or dE/dT not finite.
//
// absolute: E, dE/dT and K^E times sign(E), the derivative of |E|; exact, a multiplication by +-1.
//
// The steps are sens_core.h's (ell_sens_steps below is this header's own copy; tests/ell_sens_tolerances.py has the
// sweep that confirmed them).  Those over c and over the layer values cannot move without K_phase leaving the phase
// pass's bits.  Flat earth, fundamental mode, Rayleigh.  Compiled like sens_core.h (-ffp-contract=off), for the device
// and with g++ for the host twin (tests/hostsim/ell_sens_sim.cpp).
#pragma once
#include "ell_core.h"
#include "sens_core.h"

namespace bh {

BH_DEV SensSteps ell_sens_steps()
{
    SensSteps s;
    s.c = 0x1p-20; s.t = 0x1p-16; s.h = 0x1p-16; s.v = 0x1p-20; s.rho = 0x1p-20;
    return s;
}

// Dunkin's vector at the surface for (T, c): swd_dltar4's recursion (llw = 1) on the accessor's doubles.  Returns wvno.
template <class Lay>
BH_DEV double ell_sens_vector(const Lay &lay, int mmax, double t1, double c, double e[5])
{
    const double TWOPI = 2.0 * 3.141592653589793;
    const double omga = TWOPI / t1;
    const double wvno = omga / c;
    double omega = omga;
    if (omega < 1.0e-4) omega = 1.0e-4;
    const double wvno2 = wvno * wvno;
    swd_ray_halfspace(lay, mmax, wvno, wvno2, omega, e);
    for (int m = mmax - 1; m >= 1; m--) {       // Fortran index m; 0-based layer m-1
        Dunkin a;
        swd_ray_layer_matrix(lay, m - 1, wvno, wvno2, omega, a);
        swd_dunkin_apply(e, a);
    }
    return wvno;
}

// One pass: the period equation F (sens_F<2>'s bits) and the ratio G of the form
template <int FORM, class Lay>
BH_DEV void ell_sens_FG(const Lay &lay, int mmax, double t1, double c, double *F, double *G)
{
    double e[5];
    const double wvno = ell_sens_vector(lay, mmax, t1, c, e);
    *F = e[0];
    *G = FORM == ELL_FORM_TZ ? e[3] / (wvno * e[2]) : -wvno * e[2] / e[1];
}

// Central differences of F and of G over c (which = 0) or over T (which = 1) with the relative step r; the one of F is
// sens_diff_ct's, operation for operation
template <int FORM, class Lay>
BH_DEV void ell_sens_diff_ct(const Lay &lay, int mmax, double t1, double c, int which, double r, double &dF, double &dG)
{
    const double base = which ? t1 : c;
    const double xp = base * (1.0 + r), xm = base * (1.0 - r);
    double df = 0.0, dg = 0.0;
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const double x = s ? xm : xp;
        double f, g;
        ell_sens_FG<FORM>(lay, mmax, which ? x : t1, which ? c : x, &f, &g);
        df = s ? df - f : f;
        dg = s ? dg - g : g;
    }
    dF = df / (xp - xm);
    dG = dg / (xp - xm);
}

// What the root step leaves for the slots of a (model, period), and for the caller
struct EllSensRoot {
    double c, fc, dcdt;          // sens_root's values
    double E, gc, dE_dT;         // signed, whatever `absolute` says: the caller applies sgn
    double sgn;                  // +1, or -1 where E < 0
};

// The root step of one (model, period) from the stored phase velocity c0.  false: no value.  The caller has checked
// the model (2 <= mmax, a solid top layer) and the search's flag, as for sens_root.
template <int FORM, class Lay>
BH_DEV bool ell_sens_root(const Lay &lay, int mmax, double t1, double c0, const SensSteps &st, EllSensRoot &R)
{
    if (!(c0 > 0.0) || !(c0 < __builtin_inf())) return false;
    double c = c0;
#pragma unroll 1
    for (int it = 0; it < SENS_NEWTON; it++) {
        const double f = sens_F<2>(lay, mmax, t1, c);
        const double fc = sens_diff_ct<2>(lay, mmax, t1, c, 0, st.c);
        const double dc = f / fc;
        c = c - dc;
        if (!(fabs(dc) > SENS_STOP * c)) break;         // converged, or NaN: the test below rejects it
    }
    if (!(fabs(c - c0) <= SENS_ACCEPT * c0)) return false;
    double fc, gc, ft, gt;
    ell_sens_diff_ct<FORM>(lay, mmax, t1, c, 0, st.c, fc, gc);
    if (fc == 0.0 || fc != fc) return false;
    ell_sens_diff_ct<FORM>(lay, mmax, t1, c, 1, st.t, ft, gt);
    double e[5];
    const double wvno = ell_sens_vector(lay, mmax, t1, c, e);
    if (e[2] == 0.0) return false;                      // no vertical motion at the surface
    const double E = FORM == ELL_FORM_TZ ? e[3] / (wvno * e[2]) : -wvno * e[2] / e[1];
    const double dcdt = -ft / fc;
    const double dEdT = gt + gc * dcdt;
    const double inf = __builtin_inf();
    if (!(fabs(E) < inf) || !(fabs(gc) < inf) || !(fabs(fc) < inf) || !(fabs(dEdT) < inf)) return false;
    R.c = c; R.fc = fc; R.dcdt = dcdt;
    R.E = E; R.gc = gc; R.dE_dT = dEdT;
    R.sgn = E < 0.0 ? -1.0 : 1.0;
    return true;
}

// dE/dm of slot (kind, idx) at the polished root c with its F_c and G_c; kphase receives dc/dm in the operation order
// of sens_slot.  An entry that is zero has no relative step: 0, both.  total = false leaves the G_c dc/dm term out
// (the partial derivative at a fixed c, which depends on the form: for the tests).
template <int FORM, class Lay>
BH_DEV double ell_sens_slot(const Lay &lay, int mmax, double t1, double c, double fc, double gc, int kind, int idx,
                            const SensSteps &st, double &kphase, bool total = true)
{
    kphase = 0.0;
    // (read into scalars first: a select between members of st becomes an indexed load, and st then lives in scratch)
    const double sh = st.h, sv = st.v, srho = st.rho;
    const double r = kind == SENS_H ? sh : kind == SENS_RHO ? srho : sv;
    const double v = kind == SENS_H ? (double)lay.d(idx) : kind == SENS_VP ? (double)lay.a(idx)
                   : kind == SENS_VS ? (double)lay.b(idx) : (double)lay.rho(idx);
    const double fp = 1.0 + r, fm = 1.0 - r;
    const double dv = v * fp - v * fm;
    if (dv == 0.0) return 0.0;
    double df = 0.0, dg = 0.0;
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const SensLay<Lay> p{lay, kind, idx, s ? fm : fp};
        double f, g;
        ell_sens_FG<FORM>(p, mmax, t1, c, &f, &g);
        df = s ? df - f : f;
        dg = s ? dg - g : g;
    }
    kphase = -(df / dv) / fc;
    return total ? (dg - gc * df / fc) / dv : dg / dv;
}

}  // namespace bh
