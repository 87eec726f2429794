// ell_sens_capi.hip -- the C ABI of the ellipticity sensitivity kernels (include/bayhunter_amd.h): bh_ell_sens_batch on
// device pointers and the synchronous single-model form bh_ellipticity_sensitivity.  Host code only; the kernels are in
// ell_sens.hip.
#include <hip/hip_runtime.h>
#include <vector>
#include "ell_sens_launch.h"
#include "host_common.h"

extern "C" {

size_t bh_ell_sens_workspace_bytes(int B, int nper)
{
    if (B < 0 || nper < 0) return 0;
    return (size_t)B * (size_t)nper * bh::ELL_SENS_WS * sizeof(double);
}

int bh_ell_sens_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp, const double *vs,
                      const double *rho, int nper, const double *periods, int flsph, int absolute, const double *c,
                      int c_stride, const int *c_err, int err_stride, double *K, double *E, double *dE_dT, double *c_out,
                      double *K_phase, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return bh::fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return bh::fail_arg_("model_stride < Lmax");
    if (nper < 1 || nper > BH_MAX_PERIODS) return bh::fail_arg_("nper out of range (1 .. 60)");
    if (flsph != 0) return bh::fail_arg_("flsph: sensitivity kernels are formed on a flat earth only");
    if (c_stride < nper) return bh::fail_arg_("c_stride shorter than nper");
    if (err_stride < 1) return bh::fail_arg_("err_stride < 1");
    if (!nlay || !h || !vp || !vs || !rho || !periods || !c || !c_err || !K || !E || !dE_dT || !c_out)
        return bh::fail_arg_("NULL pointer");
    if (B == 0) return BH_OK;
    if (!workspace || workspace_bytes < bh_ell_sens_workspace_bytes(B, nper))
        return bh::fail_(BH_ERR_WORKSPACE, "workspace too small (bh_ell_sens_workspace_bytes)");
    bh::EllSensArgs A;
    A.B = B; A.Lmax = Lmax; A.nper = nper; A.mstride = model_stride; A.absolute = absolute ? 1 : 0;
    A.c_stride = c_stride; A.err_stride = err_stride;
    A.nlay = nlay; A.h = h; A.vp = vp; A.vs = vs; A.rho = rho;
    A.periods = periods; A.c = c; A.c_err = c_err;
    A.K = K; A.K_phase = K_phase; A.E = E; A.dE_dT = dE_dT; A.c_out = c_out; A.ws = (double *)workspace;
    if (!bh::ell_sens_fits(A)) return bh::fail_arg_("B * nper * 4 * Lmax lanes do not fit one launch");
    int rc = bh::require_device();
    if (rc) return rc;
    BH_HIP(bh::launch_ell_sens(A, (hipStream_t)stream));
    return BH_OK;
}

int bh_ellipticity_sensitivity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int iflsph,
                               int absolute, int kmax, const double *t, double *K, double *E, double *dE_dT, double *c_out,
                               double *K_phase, int *err)
{
    if (!thkm || !vpm || !vsm || !rhom || !t || !K || !E || !dE_dT || !c_out || !err) return bh::fail_arg_("NULL pointer");
    if (nlayer < 1 || nlayer > BH_MAX_LAYERS) return bh::fail_arg_("nlayer out of range (max 100)");
    if (kmax < 1 || kmax > BH_MAX_PERIODS) return bh::fail_arg_("kmax out of range (1 .. 60)");
    if (iflsph != 0) return bh::fail_arg_("iflsph: sensitivity kernels are formed on a flat earth only");
    // the search: fundamental-mode Rayleigh phase velocities, through the dispersion drop-in
    std::vector<double> cg(kmax);
    int rc = bh_surfdisp96(thkm, vpm, vsm, rhom, nlayer, 0, 2, 1, 0, kmax, t, cg.data(), err);
    if (rc) return rc;
    // the pass: [h|vp|vs|rho|t|c] fp64 (exactly representable fp32 layers), then [c_out|E|dE_dT|workspace|K|K_phase] and
    // [nlay, err]
    const int L = nlayer;
    std::vector<double> hb(4 * (size_t)L + 2 * (size_t)kmax);
    for (int i = 0; i < L; i++) {
        hb[i] = thkm[i]; hb[L + i] = vpm[i]; hb[2 * L + i] = vsm[i]; hb[3 * L + i] = rhom[i];
    }
    for (int k = 0; k < kmax; k++) { hb[4 * L + k] = t[k]; hb[4 * L + kmax + k] = cg[k]; }
    const size_t nK = (size_t)kmax * 4 * L, nws = (size_t)kmax * bh::ELL_SENS_WS;
    const size_t off_out = hb.size() * sizeof(double);
    const size_t off_int = off_out + (3 * (size_t)kmax + nws + 2 * nK) * sizeof(double);
    rc = bh::g_scratch.ensure(off_int + 2 * sizeof(int));
    if (rc) return rc;
    char *d = (char *)bh::g_scratch.p;
    BH_HIP(hipMemcpy(d, hb.data(), off_out, hipMemcpyHostToDevice));
    const int ints[2] = {nlayer, *err};
    BH_HIP(hipMemcpy(d + off_int, ints, sizeof(ints), hipMemcpyHostToDevice));
    const double *dm = (const double *)d;
    double *dout = (double *)(d + off_out);
    double *dws = dout + 3 * kmax, *dK = dws + nws, *dKp = dK + nK;
    rc = bh_ell_sens_batch(1, L, L, (const int *)(d + off_int), dm, dm + L, dm + 2 * L, dm + 3 * L, kmax, dm + 4 * L, 0,
                           absolute, dm + 4 * L + kmax, kmax, (const int *)(d + off_int) + 1, 1, dK, dout + kmax,
                           dout + 2 * kmax, dout, K_phase ? dKp : nullptr, dws, nws * sizeof(double), nullptr);
    if (rc) return rc;
    BH_HIP(hipDeviceSynchronize());
    BH_HIP(hipMemcpy(c_out, dout, kmax * sizeof(double), hipMemcpyDeviceToHost));
    BH_HIP(hipMemcpy(E, dout + kmax, kmax * sizeof(double), hipMemcpyDeviceToHost));
    BH_HIP(hipMemcpy(dE_dT, dout + 2 * kmax, kmax * sizeof(double), hipMemcpyDeviceToHost));
    BH_HIP(hipMemcpy(K, dK, nK * sizeof(double), hipMemcpyDeviceToHost));
    if (K_phase) BH_HIP(hipMemcpy(K_phase, dKp, nK * sizeof(double), hipMemcpyDeviceToHost));
    return BH_OK;
}

}  // extern "C"
