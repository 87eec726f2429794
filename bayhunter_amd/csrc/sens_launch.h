// sens_launch.h -- argument block and launcher of sens_root_kernel and sens_kernel, shared by sensitivity.hip and
// sens_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace bh {

struct SensArgs {
    int B, Lmax, nper;
    int mstride;             // elements between consecutive models in h/vp/vs/rho
    int iwave;               // 1 Love, 2 Rayleigh
    int c_stride, err_stride;
    const int *nlay;
    const double *h, *vp, *vs, *rho;
    const double *periods;   // [nper]
    const double *c;         // row b: c + b * c_stride, the phase velocities the search stored
    const int *c_err;        // row b: c_err[b * err_stride], the err flag of the target that wrote c
    double *K;               // [B][nper][4][Lmax]
    double *c_out, *dc_dT;   // [B][nper]
    double *fc;              // [B][nper] workspace: F_c at the polished root
};
// B * nper * 4 * Lmax lanes must fit a grid: false when they do not (nothing is launched)
bool sens_fits(const SensArgs &A);
hipError_t launch_sens(const SensArgs &A, hipStream_t stream);

}  // namespace bh
