// ell_launch.h -- argument block and launcher of ell_kernel, shared by ellipticity.hip and ell_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace bh {

struct EllArgs {
    int B, Lmax, nper;
    int mstride;             // elements between consecutive models in h/vp/vs/rho
    int flsph, absolute;
    int c_stride, err_stride, out_stride;
    const int *nlay;
    const double *h, *vp, *vs, *rho;
    const double *periods;   // [nper]
    const double *c;         // row b: c + b * c_stride, the phase velocities of the periods
    const int *c_err;        // row b: c_err[b * err_stride], the err flag of the target that wrote c
    double *out;             // row b: out + b * out_stride
};
hipError_t launch_ell(const EllArgs &A, hipStream_t stream);

}  // namespace bh
