// rf_sens_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Host twin of rf_sens_kernel (bayhunter_amd/csrc/rf_sens.hip): rf_sens_core.h compiled with g++ and the device math
// of bh_math.h (the flags of conftest's hostsim_devmath build) -- the phases of rf_core.h on a staged copy of the model
// per (slot, sign), one variant at a time, with the kernel's own conditions for a NaN and for a 0.  The steps of the
// central differences may be given, for the sweep of tests/rf_sens_tolerances.py.  With RF_SENS_SIM_MAIN a stand-alone
// program for a sanitizer run.  Never loaded by the bayhunter_amd package.
#define BH_HOSTSIM 1
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../bayhunter_amd/csrc/rf_sens_core.h"

// One row of bh_rf_sens_batch: K [nout][4][Lmax], rf [nout] or null.  h, vp, vs, rho: Lmax entries, nlay of them read;
// qp, qs: Lmax entries or null.  steps: (h, vp, vs, rho) or null for the library's.  nsv <= 0 and sigma NaN: from the top
// layer.
extern "C" void rs_rf_sens_row(int nlay, int Lmax, const double *h, const double *vp, const double *vs, const double *rho,
                               const double *qp, const double *qs, double p, double gauss, int nsamp, double fsamp,
                               double tshift, double nsv, double sigma, int waveno, int nout, const double *steps, double *K,
                               double *rf)
{
    bh::RfSensSteps st = bh::rf_sens_steps();
    if (steps) { st.h = steps[0]; st.vp = steps[1]; st.vs = steps[2]; st.rho = steps[3]; }
    bh::rf_sens_host_row(nlay, Lmax, h, vp, vs, rho, qp, qs, p, gauss, nsamp, fsamp, tshift, nsv, sigma, waveno, nout, st, K, rf);
}

extern "C" void rs_steps(double *steps)
{
    const bh::RfSensSteps st = bh::rf_sens_steps();
    steps[0] = st.h; steps[1] = st.vp; steps[2] = st.vs; steps[3] = st.rho;
}

// slot s of a model of nlay layers -> kind * 1000 + layer (the kernel's numbering)
extern "C" int rs_slot(int nlay, int s)
{
    int kind, idx;
    bh::rf_sens_slot(nlay, s, &kind, &idx);
    return kind * 1000 + idx;
}

// (+, -) pairs per workgroup of rf_sens_kernel's launch (0: the sequential form) and the LDS of that launch in bytes
extern "C" int rs_pairs(int Lmax, int nsamp) { return bh::rf_sens_pairs(Lmax, nsamp); }
extern "C" long rs_lds_bytes(int Lmax, int nsamp)
{
    const int pairs = bh::rf_sens_pairs(Lmax, nsamp);
    return (long)bh::rf_sens_lds_bytes(Lmax, nsamp, pairs ? 2 * pairs : 1);
}

#if defined(RF_SENS_SIM_MAIN)
// Crustal stacks of 2 .. 6 layers in padded rows, both wave types, and the rows without a value: every
// value read and written under the sanitizers.
int main()
{
    int finite = 0, total = 0;
    for (int n = 2; n <= 6; n++)             // (a half-space alone has no trace: 0 / 0)
        for (int waveno = 0; waveno < 2; waveno++) {
            const int L = n + 2, nout = 50;
            std::vector<double> h(L, 7.7), vp(L, 7.7), vs(L, 7.7), rho(L, 7.7), K((size_t)nout * 4 * L), rf(nout);
            for (int i = 0; i < n; i++) {
                vs[i] = 2.6 + 1.9 * i / (n > 1 ? n - 1 : 1);
                vp[i] = 1.75 * vs[i];
                rho[i] = 0.77 + 0.32 * vp[i];
                h[i] = i == n - 1 ? 0.0 : 4.0 + 3.0 * i;
            }
            rs_rf_sens_row(n, L, h.data(), vp.data(), vs.data(), rho.data(), nullptr, nullptr, 6.4, 1.0, 64, 5.0, 5.0, -1.0,
                           std::nan(""), waveno, nout, nullptr, K.data(), rf.data());
            for (int t = 0; t < nout; t++) {
                finite += std::isfinite(rf[t]); total++;
                for (int kind = 0; kind < 4; kind++)
                    for (int i = 0; i < L; i++) {
                        const double v = K[((size_t)t * 4 + kind) * L + i];
                        if (i >= n) { if (v == v) { std::printf("padding not NaN\n"); return 1; } continue; }
                        if (kind == 0 && i == n - 1 && v != 0.0) { std::printf("half-space thickness\n"); return 1; }
                        finite += std::isfinite(v); total++;
                    }
            }
            // nlay out of range: NaN throughout
            rs_rf_sens_row(L + 1, L, h.data(), vp.data(), vs.data(), rho.data(), nullptr, nullptr, 6.4, 1.0, 64, 5.0, 5.0, -1.0,
                           std::nan(""), waveno, nout, nullptr, K.data(), rf.data());
            for (double v : K) if (v == v) { std::printf("nlay out of range\n"); return 1; }
            for (int s = 0; s < 4 * n - 1; s++) {
                const int ks = rs_slot(n, s);
                if (ks / 1000 > 3 || ks % 1000 >= n || (ks / 1000 == 0 && ks % 1000 >= n - 1)) { std::printf("slot\n"); return 1; }
            }
        }
    std::printf("rf sens ok: %d of %d values finite\n", finite, total);
    return finite == total ? 0 : 1;
}
#endif
