// ell_core.h -- ellipticity (H/V) of the fundamental Rayleigh mode at a phase velocity the dispersion search found.
//
// swd_dltar4 carries Dunkin's vector e from the half-space to the free surface and returns e[0], the period equation.
// The vector is the set of 2x2 minors of the two solutions that decay in the half-space, taken over pairs of the
// motion-stress components (Ur, Uz, Tz, Tr).  The surface motion is the combination of the two solutions whose traction
// vanishes, so its horizontal-to-vertical ratio is a quotient of minors, and the common scale normc divides out:
//
//     ELL_FORM_TZ    e[3] / (wvno e[2])   = minor(Ur, Tz) / minor(Uz, Tz): the normal traction eliminated
//     ELL_FORM_TR   -wvno e[2] / e[1]     the same with the shear traction eliminated
//
// (which form eliminates which traction is what the independent reference says: tests/test_ellipticity.py compares
// each with both eliminations of tests/ellipticity_ref.py).  Positive for retrograde motion (0.6812 on a Poisson
// half-space).  The two agree at an exact root of e[0] and differ by O(dc) at the root the search returns (|dc| <=
// 1e-6 c, then rounded to real*4).  ell_eval takes ELL_FORM_TZ: it is the quantity the reference computes at the same
// c -- zero normal traction -- so that it is held to rounding error, 1e-13, and not to the search's tolerance, 1e-5 to
// 1e-2 (tests/ellipticity_tolerances.py has both forms' measured errors).
//
// One pass of the layer recursion per period, against the ~33 of the search.  Compiled like the dispersion path
// (-ffp-contract=off), for the device and with g++ for the host twin (tests/hostsim/ell_sim.cpp).
#pragma once
#include "swd_core.h"

namespace bh {

enum { ELL_FORM_TZ = 0, ELL_FORM_TR = 1 };

#if defined(BH_HOSTSIM)
#define BH_ELL_MEMBER inline
#else
#define BH_ELL_MEMBER __device__ __forceinline__
#endif

// The four real*4 values of one layer behind the accessors swd_ray_halfspace / swd_ray_layer_matrix ask a model for
// (the index is ignored): the pass reads a layer once, from wherever the model lives.
struct EllLayer {
    float vd, va, vb, vr;
    BH_ELL_MEMBER float d(int) const { return vd; }
    BH_ELL_MEMBER float a(int) const { return va; }
    BH_ELL_MEMBER float b(int) const { return vb; }
    BH_ELL_MEMBER float rho(int) const { return vr; }
};

// A model where the batched entry points keep it: four fp64 rows, rounded to real*4 as the dispersion path rounds
// them when it fetches a model (kernels.hip: QueueSrc).
struct EllModelLay {
    const double *h, *vp, *vs, *rh;
    BH_ELL_MEMBER float d(int i) const { return (float)h[i]; }
    BH_ELL_MEMBER float a(int i) const { return (float)vp[i]; }
    BH_ELL_MEMBER float b(int i) const { return (float)vs[i]; }
    BH_ELL_MEMBER float rho(int i) const { return (float)rh[i]; }
};

// Layer i of a model as the pass sees it.  The generic form reads a Lay of swd_core.h (host arrays, an LDS image:
// already transformed by swd_sphere where the target is spherical); EllSphere below transforms as it reads.
template <class Lay>
BH_DEV EllLayer ell_layer(const Lay &lay, int i, int /*mmax*/)
{
    EllLayer l;
    l.vd = lay.d(i); l.va = lay.a(i); l.vb = lay.b(i); l.vr = lay.rho(i);
    return l;
}

// Layer i (0-based) of swd_sphere's earth-flattened model for Rayleigh waves, from the untransformed layers: what
// swd_sphere(lay, mmax, 2) leaves in d/a/b/rho(i), expression by expression.  swd_sphere walks down from the surface
// with a running depth dr; the pass walks up from the half-space and has nowhere to keep a transformed model (no LDS,
// no scratch), so the running depth of layer i is summed again, in swd_sphere's order: i additions, against the ~450
// vector instructions of the layer's matrix.
template <class Lay>
BH_DEV EllLayer ell_sphere_layer(const Lay &lay, int i, int mmax)
{
    const double ar = 6370.0;
    double dr = 0.0, dr0 = 0.0;
    for (int j = 0; j <= i; j++) {
        dr0 = dr;
        dr = dr + (double)(j == mmax - 1 ? 1.0f : lay.d(j));     // swd_sphere: d(mmax) = 1 while it runs
    }
    const double r0 = ar - dr0, r1 = ar - dr;
    const double z0 = ar * log(ar / r0);
    const double z1 = ar * log(ar / r1);
    const double tmp = (ar + ar) / (r0 + r1);
    EllLayer l;
    l.vd = (i == mmax - 1) ? 0.0f : (float)(z1 - z0);
    l.va = (float)((double)lay.a(i) * tmp);
    l.vb = (float)((double)lay.b(i) * tmp);
    l.vr = lay.rho(i) * swd_powf((float)tmp, -2.275f);
    return l;
}

// An untransformed model read through the earth-flattening transformation
template <class Lay>
struct EllSphere {
    Lay lay;
};
template <class Lay>
BH_DEV EllLayer ell_layer(const EllSphere<Lay> &s, int i, int mmax) { return ell_sphere_layer(s.lay, i, mmax); }

// H/V at (wvno, omega), signed.  The recursion of swd_dltar4 (same omega clamp, same three building blocks), then the
// quotient.  NaN for fewer than two layers and for a water layer on top (llw != 1: the ratio at the sea floor is
// another observable); a NaN in the model comes out as NaN.
template <int FORM, class Lay>
BH_DEV double ell_eval_form(const Lay &lay, int mmax, double wvno, double omga)
{
    if (mmax < 2) return __builtin_nan("");
    double e[5];
    double omega = omga;
    if (omega < 1.0e-4) omega = 1.0e-4;
    const double wvno2 = wvno * wvno;
    EllLayer l = ell_layer(lay, mmax - 1, mmax);
    swd_ray_halfspace(l, mmax, wvno, wvno2, omega, e);
    for (int m = mmax - 1; m >= 1; m--) {       // Fortran index m; 0-based layer m-1
        Dunkin a;
        l = ell_layer(lay, m - 1, mmax);
        swd_ray_layer_matrix(l, m - 1, wvno, wvno2, omega, a);
        swd_dunkin_apply(e, a);
    }
    if (!(l.vb > 0.0f)) return __builtin_nan("");     // l: the top layer
    return FORM == ELL_FORM_TZ ? e[3] / (wvno * e[2]) : -wvno * e[2] / e[1];
}

template <class Lay>
BH_DEV double ell_eval(const Lay &lay, int mmax, double wvno, double omega)
{
    return ell_eval_form<ELL_FORM_TZ>(lay, mmax, wvno, omega);
}

// The value of one (model, period): c is the phase velocity a fundamental-mode Rayleigh phase target stored (a real*4
// value held in a double; 0 for a period without a root), t1 the period.  omega and wvno as swd_period_of and swd_lane
// form them.  A c that is not a positive finite number gives NaN.
template <int FORM, class Lay>
BH_DEV double ell_value_form(const Lay &lay, int mmax, double t1, double c, bool absolute)
{
    const double TWOPI = 2.0 * 3.141592653589793;
    if (!(c > 0.0) || !(c < __builtin_inf())) return __builtin_nan("");
    const double omega = TWOPI / t1;
    const double r = ell_eval_form<FORM>(lay, mmax, omega / c, omega);
    return absolute ? fabs(r) : r;
}
template <class Lay>
BH_DEV double ell_value(const Lay &lay, int mmax, double t1, double c, bool absolute)
{
    return ell_value_form<ELL_FORM_TZ>(lay, mmax, t1, c, absolute);
}

}  // namespace bh
