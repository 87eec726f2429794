// ell_launch.h -- argument blocks and launchers of ell_kernel and ell_rows_kernel, shared by ellipticity.hip,
// ell_rows.hip and ell_capi.hip.
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

// ell_rows_kernel (ell_rows.hip): the same pass with whole models per workgroup
struct EllRowsArgs {
    int B, Lmax, nper;
    int mstride;
    int flsph, absolute;
    int c_stride, err_stride, out_stride;
    int raise_flag;          // != 0: a model whose flag is 0 and whose row holds a NaN gets BH_ELL_NO_VALUE
    const int *nlay;
    const double *h, *vp, *vs, *rho;
    const double *periods;
    const double *c;
    const int *order;        // [B] slot i works on model order[i], or null: on model i
    int *err;                // row b: err[b * err_stride], read as ell_kernel's c_err, written when the flag is raised
    double *out;
};
hipError_t launch_ell_rows(const EllRowsArgs &A, hipStream_t stream);

}  // namespace bh
