// sens_group_core.h -- depth sensitivity kernels dU/dm of the fundamental-mode group velocity, Rayleigh and Love.
//
// The group velocity here is the analytic one of the polished phase-velocity root (sens_core.h),
//
//     U(T, m) = c / (1 + (T / c) dc/dT),
//
// not the reference's finite difference of two real*4 solves.  Differentiating U = c^2 / (c + T c_T) with respect to a
// layer parameter m_j at a fixed period gives (Rodi et al. 1975), with g = U / c and K^c_j = dc/dm_j,
//
//     K^U_j = dU/dm_j = g (2 - g) K^c_j(T) - g^2 T dK^c_j/dT.
//
// dK^c_j/dT is a central difference of the phase kernel between T+ = T (1 + r_g) and T- = T (1 - r_g), r_g a power of
// two (SENS_GROUP_RG; tests/sens_group_tolerances.py has the sweep on the host twin that chose it).  Each neighbouring
// period has a root, an F_c and a sens_slot of its own: nothing of sens_core.h changes, and the centre values are, bit
// for bit, what the phase pass computes.  Three recursion sets where the phase pass runs one.
//
// From the three roots also dU/dT: c_TT = (c+ - 2 c + c-) / (r_g T)^2, and with D = 1 + T c_T / c,
// D' = c_T / c + T c_TT / c - T c_T^2 / c^2:  dU/dT = c_T / D - c D' / D^2.
//
// The side roots.  No search stored them, so Newton (as in sens_root) starts from the centre root's tangent,
// c_s = c +- c_T (T+- - T), and the polished root is accepted only where |c+- - c_s| <= SENS_GROUP_WINDOW c_s.  The
// window: by Taylor's theorem the tangent misses c(T+-) by (r_g T)^2 |c_TT| / 2 at some period between, i.e. by
// kappa r_g^2 / 2 relative to c with kappa = T^2 |c_TT| / c, a dimensionless curvature of the dispersion curve.  It is
// 0.6 at the most on the six models of the tuning list, but that list is mild: over 16 384 drawn ten-layer models and
// 16 384 of 2 .. 31 layers with vs increasing downward (bayhunter_amd.synthetic.draw_models), 21 periods of 1 .. 41 s,
// it reaches 12.5 for Rayleigh and 4.0 for Love waves on the host twin -- a slow top layer of 10 .. 25 km over fast rock,
// next to the Airy phase, where U is half of c (tests/sens_group_tolerances.py: KAPPA_DRAWN).  SENS_GROUP_KAPPA = 64 is
// five times that, and the window 32 r_g^2 = 2^-19 = 1.9e-6: of the (model, period) pairs of those draws that the
// phase pass serves, 688 128 per wave type, none is lost.  What the window guards against is Newton landing on another mode:
// the search itself separates two roots only where they lie further apart than its scan step, of the order of 1e-3 c,
// 500 windows.  It is kept a function of the step so that a swept step brings its own, and its floor is the polish's
// own scatter (1e-11 c beside a crossing): r_g >= 2^-16 keeps 32 r_g^2 above 7e-9.
//
// The window also holds the centre's dc/dT to the neighbouring roots: a tangent whose slope is off by d misses by
// d r_g T, so a (model, period) passes only where T |d| / c <= 32 r_g = 7.8e-3, and U is formed from that slope.  In
// stacks with low-velocity zones a short-period wave can be trapped in a buried slow layer; the period equation at the
// surface hardly sees it, F_T / F_c there is off by per cent, and such periods have no group value although the phase
// pass returns one: 8 % of the pairs of 1024 ten-layer draws with unsorted vs for Rayleigh, 12 % for Love waves, every
// one of them with the phase pass's dc/dT further than 4e-4 c / T from the difference of two neighbouring roots.
//
// No value: where any of the three roots has none, the (model, period) has none -- U, c, dU/dT and every K are NaN
// together (bh_sens_sets_add counts a (row, period) by its c).  Flat earth, fundamental mode.  Love waves do not see
// vp: K^U_vp is exactly 0, as are the half-space's K^U_h and the padding layers (the kernels' conditions).
//
// Compiled like sens_core.h (-ffp-contract=off), for the device and with g++ for the host twin
// (tests/hostsim/sens_group_sim.cpp): every value is one lane's fixed operation sequence.
#pragma once
#include "sens_core.h"

namespace bh {

constexpr double SENS_GROUP_RG = 0x1p-12;       // relative step of the central difference of K^c over T
constexpr double SENS_GROUP_KAPPA = 64.0;       // the bound on T^2 |c_TT| / c the window is derived from
constexpr double SENS_GROUP_WINDOW = 0.5 * SENS_GROUP_KAPPA * SENS_GROUP_RG * SENS_GROUP_RG;      // 32 r_g^2 = 2^-19

// the step over T and the acceptance window of a side root that belongs to it
struct SensGroupSteps {
    double rg, window;
};
BH_DEV SensGroupSteps sens_group_steps_of(double rg)
{
    SensGroupSteps g;
    g.rg = rg;
    g.window = 0.5 * SENS_GROUP_KAPPA * rg * rg;
    return g;
}
BH_DEV SensGroupSteps sens_group_steps() { return sens_group_steps_of(SENS_GROUP_RG); }

// What sens_group_roots leaves for the slots of a (model, period)
struct SensGroupRoots {
    double c, fc, dcdt;          // the centre: sens_root's values
    double cp, fcp, cm, fcm;     // the polished roots at T+ and T- and their F_c
    double U, dU_dT;
};

// Polished root and F_c at the neighbouring period ts from the predicted start cs.  false: no value.
template <int IWAVE, class Lay>
BH_DEV bool sens_side_root(const Lay &lay, int mmax, double ts, double cs, double window, const SensSteps &st, double &c_out,
                           double &fc_out)
{
    if (!(cs > 0.0) || !(cs < __builtin_inf())) return false;
    double c = cs;
#pragma unroll 1
    for (int it = 0; it < SENS_NEWTON; it++) {
        const double f = sens_F<IWAVE>(lay, mmax, ts, c);
        const double fc = sens_diff_ct<IWAVE>(lay, mmax, ts, c, 0, st.c);
        const double dc = f / fc;
        c = c - dc;
        if (!(fabs(dc) > SENS_STOP * c)) break;         // converged, or NaN: the test below rejects it
    }
    if (!(fabs(c - cs) <= window * cs)) return false;
    const double fc = sens_diff_ct<IWAVE>(lay, mmax, ts, c, 0, st.c);
    if (fc == 0.0 || fc != fc) return false;
    c_out = c;
    fc_out = fc;
    return true;
}

// The three roots of one (model, period) from the stored phase velocity c0, U and dU/dT.  false: no value.  The
// caller has checked the model and the search's flag, as for sens_root.
template <int IWAVE, class Lay>
BH_DEV bool sens_group_roots(const Lay &lay, int mmax, double t1, double c0, const SensSteps &st, const SensGroupSteps &gs,
                             SensGroupRoots &R)
{
    double c, fc, dcdt;
    if (!sens_root<IWAVE>(lay, mmax, t1, c0, st, c, fc, dcdt)) return false;
    const double tp = t1 * (1.0 + gs.rg), tm = t1 * (1.0 - gs.rg);
    // (scalars and selects, no array: nothing is indexed at run time)
    double cp = 0.0, fcp = 0.0, cm = 0.0, fcm = 0.0;
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const double ts = s ? tm : tp;
        const double start = c + dcdt * (ts - t1);
        double cs, fs;
        if (!sens_side_root<IWAVE>(lay, mmax, ts, start, gs.window, st, cs, fs)) return false;
        if (s) { cm = cs; fcm = fs; } else { cp = cs; fcp = fs; }
    }
    const double U = c / (1.0 + (t1 / c) * dcdt);
    const double ht = gs.rg * t1;
    const double ctt = ((cp - c) + (cm - c)) / (ht * ht);
    const double D = 1.0 + t1 * dcdt / c;
    const double Dp = dcdt / c + t1 * ctt / c - t1 * dcdt * dcdt / (c * c);
    R.c = c; R.fc = fc; R.dcdt = dcdt;
    R.cp = cp; R.fcp = fcp; R.cm = cm; R.fcm = fcm;
    R.U = U;
    R.dU_dT = dcdt / D - c * Dp / (D * D);
    // finite, both: D = 0 would leave an infinite U, which bh_sens_sets_add would count
    return fabs(U) < __builtin_inf() && fabs(R.dU_dT) < __builtin_inf();
}

// The combine step: K^U from the phase kernel at T (k0), at T+ (kp) and at T- (km)
BH_DEV double sens_group_combine(double k0, double kp, double km, double t1, double tp, double tm, double c, double U)
{
    const double g = U / c;
    const double dk = (kp - km) / (tp - tm);
    return g * (2.0 - g) * k0 - g * g * t1 * dk;
}

// dU/dm of slot (kind, idx): three sens_slot evaluations and the combine.  kphase receives the phase kernel at T,
// sens_slot's own value.
template <int IWAVE, class Lay>
BH_DEV double sens_group_slot(const Lay &lay, int mmax, double t1, double rg, double c, double fc, double cp, double fcp,
                              double cm, double fcm, double U, int kind, int idx, const SensSteps &st, double &kphase)
{
    kphase = 0.0;
    if (IWAVE == 1 && kind == SENS_VP) return 0.0;
    const double tp = t1 * (1.0 + rg), tm = t1 * (1.0 - rg);
    double k0 = 0.0, kp = 0.0, km = 0.0;
#pragma unroll 1
    for (int s = 0; s < 3; s++) {
        const double ts = s == 0 ? t1 : s == 1 ? tp : tm;
        const double cr = s == 0 ? c : s == 1 ? cp : cm;
        const double fr = s == 0 ? fc : s == 1 ? fcp : fcm;
        const double k = sens_slot<IWAVE>(lay, mmax, ts, cr, fr, kind, idx, st);
        if (s == 0) k0 = k;
        else if (s == 1) kp = k;
        else km = k;
    }
    kphase = k0;
    return sens_group_combine(k0, kp, km, t1, tp, tm, c, U);
}

}  // namespace bh
