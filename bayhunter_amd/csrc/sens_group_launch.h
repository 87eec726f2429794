// sens_group_launch.h -- argument block and launcher of sens_group_root_kernel and sens_group_kernel, shared by
// sens_group.hip and sens_group_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace bh {

enum { SENS_GROUP_WS = 6 };      // doubles of workspace per (model, period)

struct SensGroupArgs {
    int B, Lmax, nper;
    int mstride;             // elements between consecutive models in h/vp/vs/rho
    int iwave;               // 1 Love, 2 Rayleigh
    int c_stride, err_stride;
    const int *nlay;
    const double *h, *vp, *vs, *rho;
    const double *periods;   // [nper]
    const double *c;         // row b: c + b * c_stride, the phase velocities the search stored
    const int *c_err;        // row b: c_err[b * err_stride], the err flag of the target that wrote c
    double *K;               // [B][nper][4][Lmax]: dU/dm
    double *K_phase;         // the same shape: dc/dm at T, or null
    double *U, *dU_dT, *c_out;   // [B][nper]
    double *ws;              // [SENS_GROUP_WS][B * nper] workspace: F_c, c+, F_c+, c-, F_c-, dc/dT
};
// B * nper * 4 * Lmax lanes must fit a grid: false when they do not (nothing is launched)
bool sens_group_fits(const SensGroupArgs &A);
hipError_t launch_sens_group(const SensGroupArgs &A, hipStream_t stream);

}  // namespace bh
