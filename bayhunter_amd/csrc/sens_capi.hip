// sens_capi.hip -- the C ABI of the phase-velocity sensitivity kernels (include/bayhunter_amd.h): bh_sens_batch on device
// pointers and the synchronous single-model form bh_sensitivity.  Host code only; the kernels are in sensitivity.hip.
#include "sens_capi_common.h"

extern "C" {

size_t bh_sens_workspace_bytes(int B, int nper)
{
    return bh::sens_pass_workspace_bytes(B, nper, 1);
}

int bh_sens_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp, const double *vs,
                  const double *rho, int iwave, int nper, const double *periods, int flsph, const double *c, int c_stride,
                  const int *c_err, int err_stride, double *K, double *c_out, double *dc_dT, void *workspace,
                  size_t workspace_bytes, void *stream)
{
    bh::SensArgs A;
    const int rc = bh::sens_pass_check(A, B, Lmax, model_stride, nlay, h, vp, vs, rho, &iwave, nper, periods, flsph, c, c_stride,
                                       c_err, err_stride, K, c_out, dc_dT != nullptr, workspace, workspace_bytes,
                                       bh_sens_workspace_bytes(B, nper), "workspace too small (bh_sens_workspace_bytes)");
    if (rc || B == 0) return rc;
    A.iwave = iwave; A.dc_dT = dc_dT; A.fc = (double *)workspace;
    BH_HIP(bh::launch_sens(A, (hipStream_t)stream));
    return BH_OK;
}

int bh_sensitivity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int iflsph,
                   int iwave, int kmax, const double *t, double *K, double *c_out, double *dc_dT, int *err)
{
    double *const out[] = {c_out, dc_dT};
    return bh::sens_pass_single(thkm, vpm, vsm, rhom, nlayer, iflsph, &iwave, kmax, t, 1, K, nullptr, out, 2, err,
                                [&](const bh::SensStaged &s) {
                                    return bh_sens_batch(1, s.L, s.L, s.nlay, s.h, s.vp, s.vs, s.rho, iwave, s.kmax, s.t, 0, s.c,
                                                         s.kmax, s.err, 1, s.K, s.out[0], s.out[1], s.ws, s.ws_bytes, nullptr);
                                });
}

}  // extern "C"
