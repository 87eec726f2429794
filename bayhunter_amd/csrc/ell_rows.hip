// ell_rows.hip -- ell_rows_kernel: ell_kernel's values with whole models per workgroup, and the flag of a model
// without an ellipticity raised in the err column of the dispersion target it reads.
//
// ell_kernel (ellipticity.hip) maps lane g of the launch to period g % nper of model g / nper: the lanes of a model
// straddle waves and workgroups, so a lane could not write the model's flag while others still read it.  Here a
// 256-thread workgroup holds G = 256 / nper whole models (nper <= 60: G >= 4; 252 of 256 threads busy at 21 periods,
// 240 at 60): thread t is period t % nper of model slot blockIdx.x * G + t / nper, threads from G * nper on and slots
// from B on compute nothing but reach the barriers.  Slot i works on model order[i] (the processing permutation of
// the dispersion launch: neighbours of like depth, so the waves of a workgroup run like trip counts of the layer
// loop), or on model i without one; the result goes to the model's own row.
//
// The flag: every thread reads its model's err word, the workgroup meets at a barrier, a thread whose value is NaN
// marks its model's slot in LDS, and behind a second barrier the model's first thread stores BH_ELL_NO_VALUE -- if the
// word was 0, a value is NaN and the caller asked for it.  Otherwise the word is not written.  One plain store per
// flagged model, no atomics, the same result at every run.  The values are ell_kernel's, bit for bit: the same
// ell_value on the same inputs under the same NaN conditions.
#include <hip/hip_runtime.h>
#include "../../include/bayhunter_amd.h"       // BH_ELL_NO_VALUE
#include "ell_core.h"
#include "ell_launch.h"

namespace bh {

constexpr int ELLR_T = 256;

__global__ __launch_bounds__(ELLR_T) void ell_rows_kernel(EllRowsArgs A)
{
    __shared__ int no_value[ELLR_T];               // [G], G = 256 at one period
    const int t = threadIdx.x;
    const int G = ELLR_T / A.nper;
    const int s = t / A.nper, k = t - s * A.nper;
    const long slot = (long)blockIdx.x * G + s;
    const bool live = s < G && slot < (long)A.B;
    long b = 0;
    int c_err = 0;
    if (live) {
        b = A.order ? (long)A.order[slot] : slot;
        c_err = A.err[b * A.err_stride];
    }
    if (t < G) no_value[t] = 0;
    __syncthreads();                               // every read of a flag word lies before every store to one
    if (live) {
        const int nl = A.nlay[b];
        double r = __builtin_nan("");
        // ell_kernel's conditions: a failed search, a model that is not of this batch's depth, no layer above the
        // half-space: NaN, and the model is not read
        if (c_err == 0 && nl >= 2 && nl <= A.Lmax) {
            const long m = b * A.mstride;
            const EllModelLay lay{A.h + m, A.vp + m, A.vs + m, A.rho + m};
            const double c = A.c[b * A.c_stride + k], t1 = A.periods[k];
            const bool absolute = A.absolute != 0;
            r = A.flsph ? ell_value(EllSphere<EllModelLay>{lay}, nl, t1, c, absolute) : ell_value(lay, nl, t1, c, absolute);
        }
        A.out[b * A.out_stride + k] = r;
        if (r != r) no_value[s] = 1;
    }
    __syncthreads();
    if (live && k == 0 && A.raise_flag && c_err == 0 && no_value[s]) A.err[b * A.err_stride] = BH_ELL_NO_VALUE;
}

hipError_t launch_ell_rows(const EllRowsArgs &A, hipStream_t stream)
{
    const int G = ELLR_T / A.nper;
    hipLaunchKernelGGL(ell_rows_kernel, dim3((unsigned)(((long)A.B + G - 1) / G)), dim3(ELLR_T), 0, stream, A);
    return hipGetLastError();
}

}  // namespace bh
