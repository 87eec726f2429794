// ell_sens_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Host twin of ell_sens_root_kernel and ell_sens_kernel (bayhunter_amd/csrc/ell_sens.hip): ell_sens_core.h compiled
// with g++ and the device math of bh_math.h, one (model, period) at a time with the kernels' own conditions for a NaN
// and for a 0.  This translation unit includes sens_sim.cpp, the phase twin, for the search that supplies c (and so also
// exports ss_sens_row and ss_sensitivity: the phase twin's bits from the same build).  The form (which traction is
// eliminated), the steps and whether the G_c dc/dm term is kept may be given: the kernels take ELL_FORM_TZ, the
// library's steps and the total derivative.  With ELL_SENS_SIM_MAIN a stand-alone program for a sanitizer run.  Never
// loaded by the bayhunter_amd package.
#include "sens_sim.cpp"
#include "../../bayhunter_amd/csrc/ell_sens_core.h"

namespace {
template <int FORM>
void ell_row(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int Lmax, int nper,
             const double *t, const double *c, int err, const bh::SensSteps &st, int absolute, bool total, double *K, double *E,
             double *dE_dT, double *c_out, double *K_phase, double *gc_out)
{
    const double nan = std::nan("");
    // ell_sens_root_kernel: the model where it lies
    const bool model = err == 0 && nlay >= 2 && nlay <= Lmax && bh::sens_model_ok(0, nlay, Lmax, vs[0]);
    std::vector<double> fc(nper, nan), gc(nper, nan), sgn(nper, nan);
    const bh::SensModelLay lay{h, vp, vs, rho};
    for (int k = 0; k < nper; k++) {
        c_out[k] = E[k] = dE_dT[k] = nan;
        bh::EllSensRoot R;
        if (model && bh::ell_sens_root<FORM>(lay, nlay, t[k], c[k], st, R)) {
            sgn[k] = absolute ? R.sgn : 1.0;
            c_out[k] = R.c; E[k] = sgn[k] * R.E; dE_dT[k] = sgn[k] * R.dE_dT; fc[k] = R.fc; gc[k] = R.gc;
        }
        if (gc_out) gc_out[k] = gc[k];
    }
    // ell_sens_kernel: the model as the workgroup's LDS image holds it
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
                        r = sgn[k] * bh::ell_sens_slot<FORM>(rows, nlay, t[k], c_out[k], fc[k], gc[k], kind, idx, st, r0, total);
                }
                K[((size_t)k * 4 + kind) * Lmax + idx] = r;
                if (K_phase) K_phase[((size_t)k * 4 + kind) * Lmax + idx] = r0;
            }
}
}  // namespace

// One row of bh_ell_sens_batch: K and K_phase (or null) [nper][4][Lmax], E, dE_dT, c_out [nper]; gc [nper] or null
// receives the workspace's G_c.  Arguments as ss_sens_row.  form: 0 ELL_FORM_TZ (the kernels'), 1 ELL_FORM_TR; total:
// 0 leaves the G_c dc/dm term out of K.
extern "C" void es_ell_row(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int Lmax, int nper,
                           const double *t, const double *c, int err, const double *steps, int form, int absolute, int total,
                           double *K, double *E, double *dE_dT, double *c_out, double *K_phase, double *gc)
{
    bh::SensSteps st = bh::ell_sens_steps();
    if (steps) { st.c = steps[0]; st.t = steps[1]; st.h = steps[2]; st.v = steps[3]; st.rho = steps[4]; }
    if (form == bh::ELL_FORM_TZ)
        ell_row<bh::ELL_FORM_TZ>(h, vp, vs, rho, nlay, Lmax, nper, t, c, err, st, absolute, total != 0, K, E, dE_dT, c_out, K_phase, gc);
    else
        ell_row<bh::ELL_FORM_TR>(h, vp, vs, rho, nlay, Lmax, nper, t, c, err, st, absolute, total != 0, K, E, dE_dT, c_out, K_phase, gc);
}

// Twin of bh_ellipticity_sensitivity: the fundamental-mode Rayleigh phase search of the model (real*4 layers), then the
// pass.  cg [kmax] receives the search's phase velocities, the return value is the search's err flag.
extern "C" int es_ell_sensitivity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int kmax,
                                  const double *t, const double *steps, int form, int absolute, int total, double *K, double *E,
                                  double *dE_dT, double *c_out, double *K_phase, double *gc, double *cg)
{
    std::vector<float> d(thkm, thkm + nlayer), a(vpm, vpm + nlayer), b(vsm, vsm + nlayer), r(rhom, rhom + nlayer);
    HostLay lay{nullptr, nullptr, nullptr, nullptr};
    bh::SwdTargetDev tg{2, 0, 1, 0, kmax, 0, 0, 0};
    std::vector<double> cws(kmax > 0 ? kmax : 1), cbws(kmax > 0 ? kmax : 1);
    OneTask src{HostLay{d.data(), a.data(), b.data(), r.data()}, nlayer, 0, -1, cg, cws.data(), cbws.data()};
    bh::swd_lane(lay, src, tg, t, 1, nullptr);
    std::vector<double> h(thkm, thkm + nlayer), vp(vpm, vpm + nlayer), vs(vsm, vsm + nlayer), rho(rhom, rhom + nlayer);
    es_ell_row(h.data(), vp.data(), vs.data(), rho.data(), nlayer, nlayer, kmax, t, cg, src.err, steps, form, absolute, total, K, E,
               dE_dT, c_out, K_phase, gc);
    return src.err;
}

// ell_core.h's value at the stored c: what ell_kernel returns for the row (flat earth)
extern "C" void es_ell_value(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int nper,
                             const double *t, const double *c, int absolute, double *out)
{
    const bh::EllModelLay lay{h, vp, vs, rho};
    for (int k = 0; k < nper; k++) out[k] = bh::ell_value(lay, nlay, t[k], c[k], absolute != 0);
}

#if defined(ELL_SENS_SIM_MAIN)
// A crustal stack of 2 .. 9 layers, five periods, both forms, with rows that have no value and a padded call: every
// value read and written under the sanitizers.
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
        for (int form = 0; form < 2; form++) {
            std::vector<double> K(5 * 4 * (size_t)n), Kp(K.size()), E(5), dE(5), c(5), gc(5), cg(5);
            const int err = es_ell_sensitivity(h.data(), vp.data(), vs.data(), rho.data(), n, 5, t, nullptr, form, 1, 1, K.data(),
                                               E.data(), dE.data(), c.data(), Kp.data(), gc.data(), cg.data());
            if (err != 0) { std::printf("search failed: n %d\n", n); return 1; }
            for (double v : K) { finite += std::isfinite(v); total++; }
            for (double v : E) { finite += std::isfinite(v); total++; }
            // the flag, c0 = 0, water on top, a padded call without K_phase
            std::vector<double> hd(h.begin(), h.end()), vpd(vp.begin(), vp.end()), vsd(vs.begin(), vs.end()),
                rd(rho.begin(), rho.end()), K2(5 * 4 * (size_t)(n + 3)), E2(5), d2(5), c2(5), cb(cg);
            cb[0] = 0.0;
            hd.resize(n + 3, 7.7); vpd.resize(n + 3, 7.7); vsd.resize(n + 3, 7.7); rd.resize(n + 3, 7.7);
            es_ell_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, 5, t, cb.data(), 0, nullptr, form, 1, 1, K2.data(),
                       E2.data(), d2.data(), c2.data(), nullptr, nullptr);
            if (!(c2[0] != c2[0]) || !(E2[0] != E2[0]) || !(c2[2] == c[2]) || !(E2[2] == E[2])) { std::printf("no-value rows\n"); return 1; }
            es_ell_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, 5, t, cg.data(), 1, nullptr, form, 0, 1, K2.data(),
                       E2.data(), d2.data(), c2.data(), nullptr, nullptr);
            if (!(E2[3] != E2[3])) { std::printf("flag\n"); return 1; }
            vsd[0] = 0.0;
            es_ell_row(hd.data(), vpd.data(), vsd.data(), rd.data(), n, n + 3, 5, t, cg.data(), 0, nullptr, form, 0, 0, K2.data(),
                       E2.data(), d2.data(), c2.data(), nullptr, nullptr);
            if (!(c2[3] != c2[3]) || !(K2[0] != K2[0])) { std::printf("water on top\n"); return 1; }
        }
    }
    std::printf("ell sens ok: %d of %d values finite\n", finite, total);
    return finite == total ? 0 : 1;
}
#endif
