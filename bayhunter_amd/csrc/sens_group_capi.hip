// sens_group_capi.hip -- the C ABI of the group-velocity sensitivity kernels (include/bayhunter_amd.h):
// bh_sens_group_batch on device pointers and the synchronous single-model form bh_group_sensitivity.  Host code only;
// the kernels are in sens_group.hip.
#include "sens_capi_common.h"

extern "C" {

size_t bh_sens_group_workspace_bytes(int B, int nper)
{
    return bh::sens_pass_workspace_bytes(B, nper, bh::SENS_GROUP_WS);
}

int bh_sens_group_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp,
                        const double *vs, const double *rho, int iwave, int nper, const double *periods, int flsph,
                        const double *c, int c_stride, const int *c_err, int err_stride, double *K, double *U_out,
                        double *dU_dT, double *c_out, double *K_phase, void *workspace, size_t workspace_bytes, void *stream)
{
    bh::SensGroupArgs A;
    const int rc = bh::sens_pass_check(A, B, Lmax, model_stride, nlay, h, vp, vs, rho, &iwave, nper, periods, flsph, c, c_stride,
                                       c_err, err_stride, K, c_out, U_out && dU_dT, workspace, workspace_bytes,
                                       bh_sens_group_workspace_bytes(B, nper),
                                       "workspace too small (bh_sens_group_workspace_bytes)");
    if (rc || B == 0) return rc;
    A.iwave = iwave; A.K_phase = K_phase; A.U = U_out; A.dU_dT = dU_dT; A.ws = (double *)workspace;
    BH_HIP(bh::launch_sens_group(A, (hipStream_t)stream));
    return BH_OK;
}

int bh_group_sensitivity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int iflsph,
                         int iwave, int kmax, const double *t, double *K, double *U_out, double *dU_dT, double *c_out,
                         double *K_phase, int *err)
{
    double *const out[] = {c_out, U_out, dU_dT};
    return bh::sens_pass_single(thkm, vpm, vsm, rhom, nlayer, iflsph, &iwave, kmax, t, bh::SENS_GROUP_WS, K, K_phase, out, 3, err,
                                [&](const bh::SensStaged &s) {
                                    return bh_sens_group_batch(1, s.L, s.L, s.nlay, s.h, s.vp, s.vs, s.rho, iwave, s.kmax, s.t, 0,
                                                               s.c, s.kmax, s.err, 1, s.K, s.out[1], s.out[2], s.out[0],
                                                               s.K_phase, s.ws, s.ws_bytes, nullptr);
                                });
}

}  // extern "C"
