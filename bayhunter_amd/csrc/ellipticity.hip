// ellipticity.hip -- ell_kernel: the ellipticity (H/V) of the fundamental Rayleigh mode for a batch of models.
//
// One lane per (model, period): lane g of the launch is period g % nper of model g / nper, so the lanes of a wave
// hold consecutive periods of one model (of up to 64 / nper + 2 neighbouring models) and their loads of a layer are
// one address per model.  Each lane runs one pass of the layer recursion of the period equation (ell_core.h) at the
// phase velocity the dispersion search stored for its period: straight-line FP64 VALU work like the layer step of
// swd_kernel, a few hundred vector instructions per layer against 32 bytes of model, so the layers are read where
// they lie -- no LDS image, no scratch.  The loop runs to the model's own nlay.
#include <hip/hip_runtime.h>
#include "ell_core.h"
#include "ell_launch.h"

namespace bh {

constexpr int ELL_T = 256;

__global__ __launch_bounds__(ELL_T) void ell_kernel(EllArgs A)
{
    const long g = (long)blockIdx.x * ELL_T + threadIdx.x;
    if (g >= (long)A.B * A.nper) return;
    const long b = g / A.nper;
    const int k = (int)(g - b * A.nper);
    const int nl = A.nlay[b];
    double r = __builtin_nan("");
    // a failed search (err 1: periods from the first without a root hold 0), a model that is not of this batch's depth
    // (err 2, BH_MODEL_BAD_DEPTH) and a stack without a layer above the half-space: NaN, and the model is not read
    if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax) {
        const long m = b * A.mstride;
        const EllModelLay lay{A.h + m, A.vp + m, A.vs + m, A.rho + m};
        const double c = A.c[b * A.c_stride + k], t1 = A.periods[k];
        const bool absolute = A.absolute != 0;
        r = A.flsph ? ell_value(EllSphere<EllModelLay>{lay}, nl, t1, c, absolute) : ell_value(lay, nl, t1, c, absolute);
    }
    A.out[b * A.out_stride + k] = r;
}

hipError_t launch_ell(const EllArgs &A, hipStream_t stream)
{
    const long n = (long)A.B * A.nper;
    hipLaunchKernelGGL(ell_kernel, dim3((unsigned)((n + ELL_T - 1) / ELL_T)), dim3(ELL_T), 0, stream, A);
    return hipGetLastError();
}

}  // namespace bh
