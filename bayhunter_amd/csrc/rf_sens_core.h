// rf_sens_core.h -- sensitivity kernels dRF(t)/dm of the receiver function: what rf_sens_kernel (rf_sens.hip) and its
// host twin (tests/hostsim/rf_sens_sim.cpp) share.
//
// RF(t; m) is an explicit function of the model -- no root to follow -- so every entry
//
//     K[t][kind][layer] = dRF(t)/dm = (RF(t; m with the entry times 1 + r) - RF(t; m with it times 1 - r)) / (v(1+r) - v(1-r))
//
// is a central difference of two traces as rf_kernel computes them (phases 1 to 4 of rf_core.h: flattening, interface
// coefficients, recursion, spectral division, Gauss filter, inverse transform, normalisation), each on a copy of the
// model's four rows with one entry perturbed.  The step r is relative and a power of two, so 1 +- r is exact; one per
// kind (tests/rf_sens_tolerances.py has the sweep on the host twin that chose them).  qp and qs are held fixed.  The
// rotation velocities phase 2 derives from the top layer (Poisson's ratio, nsv) are those of the perturbed top layer:
// the derivative is that of the trace as the library computes it.
//
// A model of nlay layers has 4 nlay - 1 slots, numbered h of layers 0 .. nlay-2 (the half-space has no thickness:
// its K_h is 0), then vp, vs, rho of layers 0 .. nlay-1.  An entry that is zero has no relative step: 0.
#pragma once
#include <cstddef>
#include "rf_core.h"
#include "sens_core.h"

namespace bh {

// relative steps of the central differences: thickness, vp, vs, density
struct RfSensSteps {
    double h, vp, vs, rho;
};
BH_HD RfSensSteps rf_sens_steps()
{
    RfSensSteps s;
    s.h = 0x1p-17; s.vp = 0x1p-19; s.vs = 0x1p-20; s.rho = 0x1p-17;
    return s;
}
BH_DEV double rf_sens_step_of(const RfSensSteps &st, int kind)
{
    const double sh = st.h, sp = st.vp, ss = st.vs, sr = st.rho;      // (scalars first: no indexed load of st)
    return kind == SENS_H ? sh : kind == SENS_VP ? sp : kind == SENS_VS ? ss : sr;
}

BH_HD int rf_sens_nslots(int nlay) { return 4 * nlay - 1; }
// slot s of a model of nlay layers: its kind (SENS_H .. SENS_RHO) and layer
BH_HD void rf_sens_slot(int nlay, int s, int *kind, int *idx)
{
    if (s < nlay - 1) { *kind = SENS_H; *idx = s; return; }
    s -= nlay - 1;
    *kind = 1 + s / nlay;
    *idx = s - (*kind - 1) * nlay;
}

// Entry e (0 .. 4L-1: row e / L, layer e % L) of the copy of model rows h, vp, vs, rho with entry (kind, idx)
// multiplied by fac; layers from nlay on are 0 (never read by the phases).
BH_DEV double rf_sens_staged(const double *BH_RESTRICT h, const double *BH_RESTRICT vp, const double *BH_RESTRICT vs,
                             const double *BH_RESTRICT rho, int L, int nlay, int e, int kind, int idx, double fac)
{
    const int row = e / L, i = e - row * L;
    if (i >= nlay) return 0.0;
    const double v = row == SENS_H ? h[i] : row == SENS_VP ? vp[i] : row == SENS_VS ? vs[i] : rho[i];
    return (row == kind && i == idx) ? v * fac : v;
}

// The entry of K from sample t of the two transformed buffers (before the normalisation qn), v the unperturbed value
BH_DEV double rf_sens_value(double qn, double sp, double sm, double v, double r)
{
    const double dv = v * (1.0 + r) - v * (1.0 - r);
    if (dv == 0.0) return 0.0;
    return (qn * (sp - sm)) / dv;
}

// The argument block of rf_sens_kernel (rf_sens.hip).  Device pointers; P as rf_kernel's launch takes it (rf_host.h:
// rf_fill_launch; P.sigma NaN: Poisson's ratio from the top layer), tw and ftab the tables of rf_kernel.
struct RfSensArgs {
    int B;
    int mstride;             // elements between consecutive models in h/vp/vs/rho
    int pairs;               // (+, -) pairs per workgroup, 0: the sequential form (set by launch_rf_sens)
    const int *nlay;
    const double *h, *vp, *vs, *rho, *qp, *qs;
    const double *tw, *ftab;
    double *K;               // [B] rows of k_stride doubles: [nout][4][Lmax]
    long k_stride;
    RfLaunch P;
    RfSensSteps st;
};
// LDS of `blocks` variants: a block laid out like a model's block in rf_kernel (rf_layout) and the variant's four rows
BH_HD size_t rf_sens_lds_bytes(int Lmax, int nsamp, int blocks)
{
    return (size_t)blocks * (rf_layout(Lmax, nsamp).per_model + 4 * Lmax) * sizeof(double);
}
// (+, -) pairs per workgroup: what pick_rf_M (rf_capi.hip) does without its co-residency term -- this kernel runs alone,
// so the budget is a quarter of a CU's 160 KiB: four workgroups of four waves per CU, one wave of each per SIMD, as many
// as rf_kernel is built to keep resident.  At most four pairs (eight blocks, rf_kernel's limit).  0: not even one pair
// fits the budget -- the sequential form, one block.
constexpr size_t kRfSensLdsBudget = 40 * 1024;
BH_HD int rf_sens_pairs(int Lmax, int nsamp)
{
    const int pairs = (int)(kRfSensLdsBudget / rf_sens_lds_bytes(Lmax, nsamp, 2));
    return pairs > 4 ? 4 : pairs;
}
#if !defined(BH_HOSTSIM)
hipError_t launch_rf_sens(const RfSensArgs &A, hipStream_t stream);
#endif

}  // namespace bh

// ---- host replay of rf_sens_kernel's workgroup program (only with -DBH_HOSTSIM) -------------------------------------
#if defined(BH_HOSTSIM)
#include <vector>
#include "rf_host.h"
namespace bh {

// One transformed buffer (before qn) of the model rows[4 L] (h | vp | vs | rho): phases 1 to 4 as rf_sens_kernel runs
// them on a staged copy.  S: rf_layout(L, nsamp).per_model doubles.
inline void rf_sens_host_trace(const RfLaunch &P, const RfLayout &lo, int nlay, int L, const double *rows, const double *qp,
                               const double *qs, const double *tw, const double *ftab, double *S)
{
    for (int k = 0; k < lo.per_model; k++) S[k] = 0.0;
    for (int i = 0; i < nlay; i++) rf_phase1_layer(S, lo, nlay, i, rows, rows + L, rows + 2 * L, rows + 3 * L, qp, qs, 0);
    for (int i = 0; i < nlay; i++) rf_phase2_interface(S, lo, P, nlay, i, rows[L], rows[2 * L]);
    for (int j = 0; j < P.nfreq; j++)
        rf_xst(S, j, j < P.nact ? rf_phase3_task(S, lo, P, nlay, j, rf_freq_load(ftab, j)) : mk(0., 0.));
    for (int i = P.nsamp / 2 + 1; i < P.nsamp; i++) rf_fft_hermitian(S, P.nsamp, i);
    rf_host_fft(S, tw, P, true);
}

// One row of bh_rf_sens_batch: K [nout][4][Lmax] and rf [nout] (or null) of model rows h, vp, vs, rho (Lmax entries
// each; qp, qs Lmax entries or null) with the launch constants of rf_fill_launch.  sigma NaN: from the top layer.
inline void rf_sens_host_row(int nlay, int Lmax, const double *h, const double *vp, const double *vs, const double *rho,
                             const double *qp, const double *qs, double p, double gauss, int nsamp, double fsamp,
                             double tshift, double nsv, double sigma, int waveno, int nout, const RfSensSteps &st,
                             double *K, double *rf)
{
    const double nan = std::nan("");
    const int L = Lmax;
    if (nlay < 1 || nlay > L) {
        for (size_t k = 0; k < (size_t)nout * 4 * L; k++) K[k] = nan;
        if (rf) for (int t = 0; t < nout; t++) rf[t] = nan;
        return;
    }
    RfLaunch P = RfLaunch();
    rf_fill_launch(P, p, gauss, nsamp, fsamp, tshift, nsv, waveno, nout);
    P.sigma = sigma;
    P.Lmax = L;
    const RfLayout lo = rf_layout(L, nsamp);
    std::vector<double> tw(2 * (size_t)nsamp), ftab((size_t)RF_FTAB * P.nfreq), rows(4 * (size_t)L), Sp(lo.per_model),
        Sm(lo.per_model);
    rf_fill_twiddles(tw.data(), nsamp);
    rf_fill_freq_table(P, ftab.data());
    for (int t = 0; t < nout; t++)
        for (int kind = 0; kind < 4; kind++)
            for (int i = 0; i < L; i++) K[((size_t)t * 4 + kind) * L + i] = (i < nlay) ? 0.0 : nan;
    if (rf) {
        for (int e = 0; e < 4 * L; e++) rows[e] = rf_sens_staged(h, vp, vs, rho, L, nlay, e, -1, -1, 1.0);
        rf_sens_host_trace(P, lo, nlay, L, rows.data(), qp, qs, tw.data(), ftab.data(), Sp.data());
        for (int t = 0; t < nout; t++) rf[t] = P.qn * Sp[2 * rf_swz(t)];
    }
    for (int s = 0; s < rf_sens_nslots(nlay); s++) {
        int kind, idx;
        rf_sens_slot(nlay, s, &kind, &idx);
        const double r = rf_sens_step_of(st, kind);
        for (int sign = 0; sign < 2; sign++) {
            for (int e = 0; e < 4 * L; e++)
                rows[e] = rf_sens_staged(h, vp, vs, rho, L, nlay, e, kind, idx, sign ? 1.0 - r : 1.0 + r);
            rf_sens_host_trace(P, lo, nlay, L, rows.data(), qp, qs, tw.data(), ftab.data(), (sign ? Sm : Sp).data());
        }
        const double v = rf_sens_staged(h, vp, vs, rho, L, nlay, kind * L + idx, -1, -1, 1.0);
        for (int t = 0; t < nout; t++)
            K[((size_t)t * 4 + kind) * L + idx] = rf_sens_value(P.qn, Sp[2 * rf_swz(t)], Sm[2 * rf_swz(t)], v, r);
    }
}

}  // namespace bh
#endif
