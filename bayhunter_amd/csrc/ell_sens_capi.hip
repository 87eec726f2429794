// ell_sens_capi.hip -- the C ABI of the ellipticity sensitivity kernels (include/bayhunter_amd.h): bh_ell_sens_batch on
// device pointers and the synchronous single-model form bh_ellipticity_sensitivity.  Host code only; the kernels are in
// ell_sens.hip.
#include "sens_capi_common.h"

extern "C" {

size_t bh_ell_sens_workspace_bytes(int B, int nper)
{
    return bh::sens_pass_workspace_bytes(B, nper, bh::ELL_SENS_WS);
}

int bh_ell_sens_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp, const double *vs,
                      const double *rho, int nper, const double *periods, int flsph, int absolute, const double *c,
                      int c_stride, const int *c_err, int err_stride, double *K, double *E, double *dE_dT, double *c_out,
                      double *K_phase, void *workspace, size_t workspace_bytes, void *stream)
{
    bh::EllSensArgs A;
    const int rc = bh::sens_pass_check(A, B, Lmax, model_stride, nlay, h, vp, vs, rho, nullptr, nper, periods, flsph, c, c_stride,
                                       c_err, err_stride, K, c_out, E && dE_dT, workspace, workspace_bytes,
                                       bh_ell_sens_workspace_bytes(B, nper), "workspace too small (bh_ell_sens_workspace_bytes)");
    if (rc || B == 0) return rc;
    A.absolute = absolute ? 1 : 0; A.K_phase = K_phase; A.E = E; A.dE_dT = dE_dT; A.ws = (double *)workspace;
    BH_HIP(bh::launch_ell_sens(A, (hipStream_t)stream));
    return BH_OK;
}

int bh_ellipticity_sensitivity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int iflsph,
                               int absolute, int kmax, const double *t, double *K, double *E, double *dE_dT, double *c_out,
                               double *K_phase, int *err)
{
    double *const out[] = {c_out, E, dE_dT};
    return bh::sens_pass_single(thkm, vpm, vsm, rhom, nlayer, iflsph, nullptr, kmax, t, bh::ELL_SENS_WS, K, K_phase, out, 3, err,
                                [&](const bh::SensStaged &s) {
                                    return bh_ell_sens_batch(1, s.L, s.L, s.nlay, s.h, s.vp, s.vs, s.rho, s.kmax, s.t, 0, absolute,
                                                             s.c, s.kmax, s.err, 1, s.K, s.out[1], s.out[2], s.out[0], s.K_phase,
                                                             s.ws, s.ws_bytes, nullptr);
                                });
}

}  // extern "C"
