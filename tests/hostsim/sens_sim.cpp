// sens_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Host twin of sens_root_kernel and sens_kernel (bayhunter_amd/csrc/sensitivity.hip): sens_core.h compiled with g++
// and the device math of bh_math.h (the flags of conftest's hostsim_devmath build), one (model, period) at a time with
// the kernels' own conditions for a NaN and for a 0.  Also the search that supplies c (swd_lane, as
// tests/hostsim/hostsim.cpp runs it), so that ss_sensitivity is the twin of bh_sensitivity.  The steps of the central
// differences may be given, for the sweep of tests/sensitivity_tolerances.py.  With SENS_SIM_MAIN a stand-alone program
// for a sanitizer run.  Never loaded by the bayhunter_amd package.
#define BH_HOSTSIM 1
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../bayhunter_amd/csrc/sens_core.h"

namespace {
struct HostLay {
    float *pd, *pa, *pb, *pr;
    float d(int i) const { return pd[i]; }
    float a(int i) const { return pa[i]; }
    float b(int i) const { return pb[i]; }
    float rho(int i) const { return pr[i]; }
    void set_d(int i, float v) { pd[i] = v; }
    void set_a(int i, float v) { pa[i] = v; }
    void set_b(int i, float v) { pb[i] = v; }
    void set_rho(int i, float v) { pr[i] = v; }
};
struct OneTask {
    HostLay src;
    int nlayer, taken = 0, err = -1;
    double *out, *cws, *cbws;
    int next(HostLay &lay, double *&o, double *&c, double *&cb)
    {
        if (taken) return 0;
        taken = 1;
        lay = src;
        o = out; c = cws; cb = cbws;
        return nlayer;
    }
    void done(int e) { err = e; }
    void sphere(HostLay &lay, int mmax, int ifunc) { bh::swd_sphere(lay, mmax, ifunc); }
    void put(bh::SwdState &S, int k, int kmax, float v) { bh::swd_put_direct(S, k, kmax, v); }
    void fill_zero(bh::SwdState &S, int k, int kmax) { bh::swd_zero_direct(S, k, kmax); }
};

template <int IWAVE>
void one_row(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int Lmax, int nper,
             const double *t, const double *c, int err, const bh::SensSteps &st, double *K, double *c_out, double *dc_dT)
{
    const double nan = std::nan("");
    // sens_root_kernel: the model where it lies
    const bool model = err == 0 && nlay >= 2 && nlay <= Lmax && bh::sens_model_ok(0, nlay, Lmax, vs[0]);
    std::vector<double> fc(nper, nan);
    const bh::SensModelLay lay{h, vp, vs, rho};
    for (int k = 0; k < nper; k++) {
        c_out[k] = dc_dT[k] = nan;
        double c1, fc1, d1;
        if (model && bh::sens_root<IWAVE>(lay, nlay, t[k], c[k], st, c1, fc1, d1)) { c_out[k] = c1; fc[k] = fc1; dc_dT[k] = d1; }
    }
    // sens_kernel: the model as the workgroup's LDS image holds it
    std::vector<double> img(4 * (size_t)Lmax, 0.0);
    if (err == 0 && nlay >= 2 && nlay <= Lmax)
        for (int i = 0; i < nlay; i++) {
            img[i] = (double)(float)h[i]; img[Lmax + i] = (double)(float)vp[i];
            img[2 * Lmax + i] = (double)(float)vs[i]; img[3 * Lmax + i] = (double)(float)rho[i];
        }
    const bh::SensRows rows{img.data(), Lmax};
    for (int k = 0; k < nper; k++)
        for (int kind = 0; kind < 4; kind++)
            for (int idx = 0; idx < Lmax; idx++) {
                double r;
                if (c_out[k] != c_out[k]) r = nan;
                else {
                    r = 0.0;
                    if (idx < nlay && !(kind == bh::SENS_H && idx == nlay - 1))
                        r = bh::sens_slot<IWAVE>(rows, nlay, t[k], c_out[k], fc[k], kind, idx, st);
                }
                K[((size_t)k * 4 + kind) * Lmax + idx] = r;
            }
}
}  // namespace

// One row of bh_sens_batch: K [nper][4][Lmax], c_out and dc_dT [nper].  h/vp/vs/rho fp64 with nlay valid entries (Lmax:
// the call's depth), c the row's phase velocities, err its flag.  steps: null for the library's, or the five relative
// steps (c, T, h, velocities, density).
extern "C" void ss_sens_row(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int Lmax,
                            int iwave, int nper, const double *t, const double *c, int err, const double *steps, double *K,
                            double *c_out, double *dc_dT)
{
    bh::SensSteps st = bh::sens_steps();
    if (steps) { st.c = steps[0]; st.t = steps[1]; st.h = steps[2]; st.v = steps[3]; st.rho = steps[4]; }
    if (iwave == 2) one_row<2>(h, vp, vs, rho, nlay, Lmax, nper, t, c, err, st, K, c_out, dc_dT);
    else one_row<1>(h, vp, vs, rho, nlay, Lmax, nper, t, c, err, st, K, c_out, dc_dT);
}

// Twin of bh_sensitivity: the fundamental-mode phase search of the model (real*4 layers), then the pass.  cg [kmax]
// receives the search's phase velocities, the return value is the search's err flag.
extern "C" int ss_sensitivity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int iwave,
                              int kmax, const double *t, double *K, double *c_out, double *dc_dT, double *cg)
{
    std::vector<float> d(thkm, thkm + nlayer), a(vpm, vpm + nlayer), b(vsm, vsm + nlayer), r(rhom, rhom + nlayer);
    HostLay lay{nullptr, nullptr, nullptr, nullptr};
    bh::SwdTargetDev tg{iwave, 0, 1, 0, kmax, 0, 0, 0};
    std::vector<double> cws(kmax > 0 ? kmax : 1), cbws(kmax > 0 ? kmax : 1);
    OneTask src{HostLay{d.data(), a.data(), b.data(), r.data()}, nlayer, 0, -1, cg, cws.data(), cbws.data()};
    bh::swd_lane(lay, src, tg, t, 1, nullptr);
    std::vector<double> h(thkm, thkm + nlayer), vp(vpm, vpm + nlayer), vs(vsm, vsm + nlayer), rho(rhom, rhom + nlayer);
    ss_sens_row(h.data(), vp.data(), vs.data(), rho.data(), nlayer, nlayer, iwave, kmax, t, cg, src.err, nullptr, K, c_out,
                dc_dT);
    return src.err;
}

#if defined(SENS_SIM_MAIN)
// A crustal stack of 2 .. 9 layers, both wave types, five periods, with the rows that have no value: every value read
// and written under the sanitizers.
int main()
{
    const double t[5] = {1.0, 2.0, 4.0, 8.0, 12.0};
    int finite = 0, total = 0;
    for (int n = 2; n <= 9; n++) {
        std::vector<float> h(n), vp(n), vs(n), rho(n);
        for (int i = 0; i < n; i++) {
            vs[i] = 2.0f + 2.5f * i / (n - 1);
            vp[i] = 1.75f * vs[i];
            rho[i] = 0.77f + 0.32f * vp[i];
            h[i] = i == n - 1 ? 0.0f : 5.0f + i;
        }
        for (int iwave = 1; iwave <= 2; iwave++) {
            std::vector<double> K(5 * 4 * (size_t)n), c(5), dcdt(5), cg(5);
            const int err = ss_sensitivity(h.data(), vp.data(), vs.data(), rho.data(), n, iwave, 5, t, K.data(), c.data(),
                                           dcdt.data(), cg.data());
            for (double v : K) { finite += std::isfinite(v); total++; }
            if (err != 0) { std::printf("search failed: n %d iwave %d\n", n, iwave); return 1; }
            // the no-value rows: the flag, water on top, c0 = 0, a c0 moved off the root, a padded call
            std::vector<double> hd(h.begin(), h.end()), vpd(vp.begin(), vp.end()), vsd(vs.begin(), vs.end()),
                rd(rho.begin(), rho.end()), K2(5 * 4 * (size_t)(n + 3)), c2(5), d2(5), cb(cg);
            ss_sens_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n, iwave, 5, t, cg.data(), 1, nullptr, K.data(),
                        c2.data(), d2.data());
            cb[0] = 0.0; cb[1] *= 1.0 + 1e-5;
            hd.resize(n + 3, 7.7); vpd.resize(n + 3, 7.7); vsd.resize(n + 3, 7.7); rd.resize(n + 3, 7.7);
            ss_sens_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, iwave, 5, t, cb.data(), 0, nullptr, K2.data(),
                        c2.data(), d2.data());
            if (!(c2[0] != c2[0]) || !(c2[1] != c2[1]) || !(c2[2] == c[2])) { std::printf("no-value rows\n"); return 1; }
            vsd[0] = 0.0;
            ss_sens_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, iwave, 5, t, cg.data(), 0, nullptr, K2.data(),
                        c2.data(), d2.data());
            if (!(c2[3] != c2[3])) { std::printf("water on top\n"); return 1; }
        }
    }
    std::printf("sens ok: %d of %d kernel values finite\n", finite, total);
    return finite == total ? 0 : 1;
}
#endif
