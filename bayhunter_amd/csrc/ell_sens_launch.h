// ell_sens_launch.h -- argument block and launcher of ell_sens_root_kernel and ell_sens_kernel, shared by ell_sens.hip
// and ell_sens_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace bh {

enum { ELL_SENS_WS = 3 };      // doubles of workspace per (model, period): F_c, G_c, sign(E) or 1

struct EllSensArgs {
    int B, Lmax, nper;
    int mstride;             // elements between consecutive models in h/vp/vs/rho
    int absolute;            // != 0: E, dE/dT and K times sign(E)
    int c_stride, err_stride;
    const int *nlay;
    const double *h, *vp, *vs, *rho;
    const double *periods;   // [nper]
    const double *c;         // row b: c + b * c_stride, the phase velocities the search stored
    const int *c_err;        // row b: c_err[b * err_stride], the err flag of the target that wrote c
    double *K;               // [B][nper][4][Lmax] dE/dm
    double *K_phase;         // the same shape, dc/dm; or null
    double *E, *dE_dT, *c_out;       // [B][nper]
    double *ws;              // [ELL_SENS_WS][B][nper] workspace
};
// B * nper * 4 * Lmax lanes must fit a grid: false when they do not (nothing is launched)
bool ell_sens_fits(const EllSensArgs &A);
hipError_t launch_ell_sens(const EllSensArgs &A, hipStream_t stream);

}  // namespace bh
