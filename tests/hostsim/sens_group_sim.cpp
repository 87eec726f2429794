// sens_group_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Host twin of sens_group_root_kernel and sens_group_kernel (bayhunter_amd/csrc/sens_group.hip): sens_group_core.h
// compiled with g++ and the device math of bh_math.h, one (model, period) at a time with the kernels' own conditions
// for a NaN and for a 0.  This translation unit includes sens_sim.cpp, the phase twin, for the search that supplies c
// (and so also exports ss_sens_row and ss_sensitivity: the phase twin's bits from the same build).  The step r_g and
// the acceptance window may be given, for the sweep of tests/sens_group_tolerances.py and for a rejected side root.
// With SENS_GROUP_SIM_MAIN a stand-alone program for a sanitizer run.  Never loaded by the bayhunter_amd package.
#include "sens_sim.cpp"
#include "../../bayhunter_amd/csrc/sens_group_core.h"

namespace {
template <int IWAVE>
void group_row(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int Lmax, int nper,
               const double *t, const double *c, int err, const bh::SensSteps &st, const bh::SensGroupSteps &gs, double *K,
               double *U, double *dU_dT, double *c_out, double *K_phase, double *dc_dT)
{
    const double nan = std::nan("");
    // sens_group_root_kernel: the model where it lies
    const bool model = err == 0 && nlay >= 2 && nlay <= Lmax && bh::sens_model_ok(0, nlay, Lmax, vs[0]);
    std::vector<bh::SensGroupRoots> R(nper);
    const bh::SensModelLay lay{h, vp, vs, rho};
    for (int k = 0; k < nper; k++) {
        bh::SensGroupRoots R1;
        R[k].c = R[k].fc = R[k].dcdt = R[k].cp = R[k].fcp = R[k].cm = R[k].fcm = R[k].U = R[k].dU_dT = nan;
        if (model && bh::sens_group_roots<IWAVE>(lay, nlay, t[k], c[k], st, gs, R1)) R[k] = R1;
        c_out[k] = R[k].c; U[k] = R[k].U; dU_dT[k] = R[k].dU_dT;
        if (dc_dT) dc_dT[k] = R[k].dcdt;
    }
    // sens_group_kernel: the model as the workgroup's LDS image holds it
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
                double r, r0;
                if (c_out[k] != c_out[k]) r = r0 = nan;
                else {
                    r = r0 = 0.0;
                    if (idx < nlay && !(kind == bh::SENS_H && idx == nlay - 1))
                        r = bh::sens_group_slot<IWAVE>(rows, nlay, t[k], gs.rg, R[k].c, R[k].fc, R[k].cp, R[k].fcp, R[k].cm,
                                                       R[k].fcm, R[k].U, kind, idx, st, r0);
                }
                K[((size_t)k * 4 + kind) * Lmax + idx] = r;
                if (K_phase) K_phase[((size_t)k * 4 + kind) * Lmax + idx] = r0;
            }
}
}  // namespace

// One row of bh_sens_group_batch: K and K_phase (or null) [nper][4][Lmax], U, dU_dT, c_out [nper]; dc_dT [nper] or null
// receives the workspace's dc/dT.  Arguments as ss_sens_row.  rg: the step over T, or <= 0 for the library's; window:
// the acceptance window of the side roots, or < 0 for the one that belongs to the step.
extern "C" void sg_group_row(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int Lmax,
                             int iwave, int nper, const double *t, const double *c, int err, const double *steps, double rg,
                             double window, double *K, double *U, double *dU_dT, double *c_out, double *K_phase, double *dc_dT)
{
    bh::SensSteps st = bh::sens_steps();
    if (steps) { st.c = steps[0]; st.t = steps[1]; st.h = steps[2]; st.v = steps[3]; st.rho = steps[4]; }
    bh::SensGroupSteps gs = rg > 0.0 ? bh::sens_group_steps_of(rg) : bh::sens_group_steps();
    if (window >= 0.0) gs.window = window;
    if (iwave == 2) group_row<2>(h, vp, vs, rho, nlay, Lmax, nper, t, c, err, st, gs, K, U, dU_dT, c_out, K_phase, dc_dT);
    else group_row<1>(h, vp, vs, rho, nlay, Lmax, nper, t, c, err, st, gs, K, U, dU_dT, c_out, K_phase, dc_dT);
}

// Twin of bh_group_sensitivity: the fundamental-mode phase search of the model (real*4 layers), then the pass.  cg [kmax]
// receives the search's phase velocities, the return value is the search's err flag.
extern "C" int sg_group_sensitivity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer,
                                    int iwave, int kmax, const double *t, double rg, double window, double *K, double *U,
                                    double *dU_dT, double *c_out, double *K_phase, double *dc_dT, double *cg)
{
    std::vector<float> d(thkm, thkm + nlayer), a(vpm, vpm + nlayer), b(vsm, vsm + nlayer), r(rhom, rhom + nlayer);
    HostLay lay{nullptr, nullptr, nullptr, nullptr};
    bh::SwdTargetDev tg{iwave, 0, 1, 0, kmax, 0, 0, 0};
    std::vector<double> cws(kmax > 0 ? kmax : 1), cbws(kmax > 0 ? kmax : 1);
    OneTask src{HostLay{d.data(), a.data(), b.data(), r.data()}, nlayer, 0, -1, cg, cws.data(), cbws.data()};
    bh::swd_lane(lay, src, tg, t, 1, nullptr);
    std::vector<double> h(thkm, thkm + nlayer), vp(vpm, vpm + nlayer), vs(vsm, vsm + nlayer), rho(rhom, rhom + nlayer);
    sg_group_row(h.data(), vp.data(), vs.data(), rho.data(), nlayer, nlayer, iwave, kmax, t, cg, src.err, nullptr, rg, window,
                 K, U, dU_dT, c_out, K_phase, dc_dT);
    return src.err;
}

#if defined(SENS_GROUP_SIM_MAIN)
// A crustal stack of 2 .. 9 layers, both wave types, five periods, with rows that have no value and a padded call:
// every value read and written under the sanitizers.
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
            std::vector<double> K(5 * 4 * (size_t)n), Kp(K.size()), U(5), dU(5), c(5), cg(5);
            const int err = sg_group_sensitivity(h.data(), vp.data(), vs.data(), rho.data(), n, iwave, 5, t, 0.0, -1.0, K.data(),
                                                 U.data(), dU.data(), c.data(), Kp.data(), nullptr, cg.data());
            if (err != 0) { std::printf("search failed: n %d iwave %d\n", n, iwave); return 1; }
            for (double v : K) { finite += std::isfinite(v); total++; }
            for (double v : U) { finite += std::isfinite(v); total++; }
            // the flag, c0 = 0, a window nothing passes, a padded call without K_phase
            std::vector<double> hd(h.begin(), h.end()), vpd(vp.begin(), vp.end()), vsd(vs.begin(), vs.end()),
                rd(rho.begin(), rho.end()), K2(5 * 4 * (size_t)(n + 3)), U2(5), d2(5), c2(5), cb(cg);
            cb[0] = 0.0;
            hd.resize(n + 3, 7.7); vpd.resize(n + 3, 7.7); vsd.resize(n + 3, 7.7); rd.resize(n + 3, 7.7);
            sg_group_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, iwave, 5, t, cb.data(), 0, nullptr, 0.0, -1.0,
                         K2.data(), U2.data(), d2.data(), c2.data(), nullptr, nullptr);
            if (!(c2[0] != c2[0]) || !(U2[0] != U2[0]) || !(c2[2] == c[2]) || !(U2[2] == U[2])) { std::printf("no-value rows\n"); return 1; }
            sg_group_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, iwave, 5, t, cg.data(), 0, nullptr, 0.0, 0.0,
                         K2.data(), U2.data(), d2.data(), c2.data(), nullptr, nullptr);
            if (!(c2[1] != c2[1]) || !(K2[0] != K2[0])) { std::printf("rejected side root\n"); return 1; }
            sg_group_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, iwave, 5, t, cg.data(), 1, nullptr, 0.0, -1.0,
                         K2.data(), U2.data(), d2.data(), c2.data(), nullptr, nullptr);
            if (!(U2[3] != U2[3])) { std::printf("flag\n"); return 1; }
        }
    }
    std::printf("sens group ok: %d of %d values finite\n", finite, total);
    return finite == total ? 0 : 1;
}
#endif
