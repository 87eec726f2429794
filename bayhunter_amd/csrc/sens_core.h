// sens_core.h -- depth sensitivity kernels dc/dm of the fundamental-mode phase velocity, Rayleigh and Love.
//
// The period equation F(c, T, m) = swd_dltar4 / swd_dltar1 (swd_core.h) vanishes at the phase velocity c of period T in
// the model m.  By the implicit-function theorem
//
//     dc/dm_j = -F_mj / F_c        dc/dT = -F_T / F_c        at F = 0,
//
// with every partial derivative a central difference of F.  The recursions are templates over a layer accessor and cast
// what it returns to double, so SensLay below -- an accessor that returns doubles, one of them perturbed -- gives the
// period equation of a perturbed model without a change to the solver.  The layers are the real*4 values the search
// saw, promoted to double: the derivatives belong to the model whose root the search returned.
//
// normc and the Love recursion's normalisation scale F by a positive factor that depends on (c, T, m) continuously.
// At a root that leaves every quotient above unchanged; away from it the quotients move by O(F).  The search stops at
// a bracket of 1e-6 c and rounds to real*4, so the root is polished first: Newton on F in c with the slope from a
// central difference, at most SENS_NEWTON steps, until |dc| <= 2^-50 c.  The bracket held the root, so a polished
// root further than SENS_ACCEPT c0 from the stored c0 is another root and the (model, period) has no value.
//
// Where c lies next to the vs of a finite layer the accuracy of all this drops: on the hyperbolic side swd_var and
// swd_love_layer form (1 - exp(-2q)) / 2 with an absolute error of 2^-54 whatever q is, and q vanishes at the crossing.
// With c on that vs the polished root is within 1e-11 of the exact one instead of 5e-16; with c, or c one step of the
// differences over c and the velocities away from it, every value loses three digits and the crossed layer's own
// dc/dvs up to five.  From |c / vs - 1| = 2^-16 outward nothing of it is left (tests/sensitivity_tolerances.py).
//
// One whole recursion per evaluation: 3 per Newton step, 4 for F_c and F_T, 2 per slot; O(L^2) per (model, period).
// The prefix / suffix form that makes it O(L) is not attempted here.
//
// Flattened earth: the derivative through swd_sphere's transformation is not formed; the entry points refuse flsph = 1.
//
// The steps are relative and powers of two (so 1 +- r is exact), one per kind; tests/sensitivity_tolerances.py has the
// sweep on the host twin that chose them.  Compiled like the dispersion path (-ffp-contract=off), for the device and
// with g++ for the host twin (tests/hostsim/sens_sim.cpp): every value is one lane's fixed operation sequence.
#pragma once
#include "swd_core.h"

namespace bh {

enum { SENS_H = 0, SENS_VP = 1, SENS_VS = 2, SENS_RHO = 3 };      // the slot kinds, in the order of K's third axis
enum { SENS_NEWTON = 4 };
constexpr double SENS_ACCEPT = 2.0e-6;          // |c - c0| <= SENS_ACCEPT c0: the search's bracket (1e-6 c) and its rounding
constexpr double SENS_STOP = 0x1p-50;

// relative steps of the central differences: c, T, thickness, velocities, density
struct SensSteps {
    double c, t, h, v, rho;
};
BH_DEV SensSteps sens_steps()
{
    SensSteps s;
    s.c = 0x1p-20; s.t = 0x1p-16; s.h = 0x1p-16; s.v = 0x1p-20; s.rho = 0x1p-20;
    return s;
}

#if defined(BH_HOSTSIM)
#define BH_SENS_MEMBER inline
#else
#define BH_SENS_MEMBER __device__ __forceinline__
#endif

// A model held as four rows of doubles that are real*4 values (an LDS image on the device)
struct SensRows {
    const double *p;        // [h | vp | vs | rho], L entries each
    int L;
    BH_SENS_MEMBER double d(int i) const { return p[i]; }
    BH_SENS_MEMBER double a(int i) const { return p[L + i]; }
    BH_SENS_MEMBER double b(int i) const { return p[2 * L + i]; }
    BH_SENS_MEMBER double rho(int i) const { return p[3 * L + i]; }
};

// A model where the batched entry point keeps it: four fp64 rows, rounded to real*4 as the dispersion path rounds them
struct SensModelLay {
    const double *h, *vp, *vs, *rh;
    BH_SENS_MEMBER double d(int i) const { return (double)(float)h[i]; }
    BH_SENS_MEMBER double a(int i) const { return (double)(float)vp[i]; }
    BH_SENS_MEMBER double b(int i) const { return (double)(float)vs[i]; }
    BH_SENS_MEMBER double rho(int i) const { return (double)(float)rh[i]; }
};

// Lay with entry (kind, idx) multiplied by fac
template <class Lay>
struct SensLay {
    Lay lay;
    int kind, idx;
    double fac;
    BH_SENS_MEMBER double d(int i) const { const double v = (double)lay.d(i); return (kind == SENS_H && i == idx) ? v * fac : v; }
    BH_SENS_MEMBER double a(int i) const { const double v = (double)lay.a(i); return (kind == SENS_VP && i == idx) ? v * fac : v; }
    BH_SENS_MEMBER double b(int i) const { const double v = (double)lay.b(i); return (kind == SENS_VS && i == idx) ? v * fac : v; }
    BH_SENS_MEMBER double rho(int i) const { const double v = (double)lay.rho(i); return (kind == SENS_RHO && i == idx) ? v * fac : v; }
};

// The period equation at (T, c): omega as swd_period_of forms it for a phase target.  IWAVE: 1 Love, 2 Rayleigh.
template <int IWAVE, class Lay>
BH_DEV double sens_F(const Lay &lay, int mmax, double t1, double c)
{
    const double TWOPI = 2.0 * 3.141592653589793;
    const double omega = TWOPI / t1;
    const double wvno = omega / c;
    return IWAVE == 2 ? swd_dltar4(lay, mmax, 1, wvno, omega) : swd_dltar1(lay, mmax, 1, wvno, omega);
}

// Central difference of F over c (which = 0) or over T (which = 1) with the relative step r
template <int IWAVE, class Lay>
BH_DEV double sens_diff_ct(const Lay &lay, int mmax, double t1, double c, int which, double r)
{
    const double base = which ? t1 : c;
    const double xp = base * (1.0 + r), xm = base * (1.0 - r);
    double df = 0.0;
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const double x = s ? xm : xp;
        const double f = sens_F<IWAVE>(lay, mmax, which ? x : t1, which ? c : x);
        df = s ? df - f : f;
    }
    return df / (xp - xm);
}

// Polished root, F_c and dc/dT of one (model, period) from the stored phase velocity c0.  false: no value (c0 not a
// positive finite number, the polish rejected, F_c zero or NaN).  The caller has checked the model (2 <= mmax, a solid
// top layer) and the search's flag.
template <int IWAVE, class Lay>
BH_DEV bool sens_root(const Lay &lay, int mmax, double t1, double c0, const SensSteps &st, double &c_out, double &fc_out,
                      double &dcdt_out)
{
    if (!(c0 > 0.0) || !(c0 < __builtin_inf())) return false;
    double c = c0;
#pragma unroll 1
    for (int it = 0; it < SENS_NEWTON; it++) {
        const double f = sens_F<IWAVE>(lay, mmax, t1, c);
        const double fc = sens_diff_ct<IWAVE>(lay, mmax, t1, c, 0, st.c);
        const double dc = f / fc;
        c = c - dc;
        if (!(fabs(dc) > SENS_STOP * c)) break;         // converged, or NaN: the test below rejects it
    }
    if (!(fabs(c - c0) <= SENS_ACCEPT * c0)) return false;
    const double fc = sens_diff_ct<IWAVE>(lay, mmax, t1, c, 0, st.c);
    if (fc == 0.0 || fc != fc) return false;
    const double ft = sens_diff_ct<IWAVE>(lay, mmax, t1, c, 1, st.t);
    c_out = c;
    fc_out = fc;
    dcdt_out = -ft / fc;
    return true;
}

// dc/dm of slot (kind, idx) at the polished root c with its F_c.  Love waves do not see vp: 0.  An entry that is zero
// has no relative step: 0.
template <int IWAVE, class Lay>
BH_DEV double sens_slot(const Lay &lay, int mmax, double t1, double c, double fc, int kind, int idx, const SensSteps &st)
{
    if (IWAVE == 1 && kind == SENS_VP) return 0.0;
    // (read into scalars first: a select between members of st becomes an indexed load, and st then lives in scratch)
    const double sh = st.h, sv = st.v, srho = st.rho;
    const double r = kind == SENS_H ? sh : kind == SENS_RHO ? srho : sv;
    const double v = kind == SENS_H ? (double)lay.d(idx) : kind == SENS_VP ? (double)lay.a(idx)
                   : kind == SENS_VS ? (double)lay.b(idx) : (double)lay.rho(idx);
    const double fp = 1.0 + r, fm = 1.0 - r;
    const double dv = v * fp - v * fm;
    if (dv == 0.0) return 0.0;
    double df = 0.0;
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const SensLay<Lay> p{lay, kind, idx, s ? fm : fp};
        const double f = sens_F<IWAVE>(p, mmax, t1, c);
        df = s ? df - f : f;
    }
    return -(df / dv) / fc;
}

// Does (model row, flag) have a value at all: the search succeeded, 2 .. Lmax layers, a solid top layer
BH_DEV bool sens_model_ok(int err, int nlay, int Lmax, double vs_top)
{
    return err == 0 && nlay >= 2 && nlay <= Lmax && (float)vs_top > 0.0f;
}

}  // namespace bh
