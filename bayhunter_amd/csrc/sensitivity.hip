// sensitivity.hip -- sens_root_kernel and sens_kernel: the sensitivity kernels dc/dm of the fundamental-mode phase
// velocity for a batch of models (sens_core.h).
//
// sens_root_kernel, one lane per (model, period) like ell_kernel: lane g is period g % nper of model g / nper.  It
// polishes the root the search stored and writes c, F_c and dc/dT: up to 3 SENS_NEWTON + 4 recursions of straight-line
// FP64 work per lane against 32 bytes of model per layer, so the layers are read where they lie.
//
// sens_kernel, one lane per (model, period, slot) with the slot the fastest index: lane g is slot g % (4 Lmax) of
// (model, period) g / (4 Lmax), so the 64 lanes of a wave hold the slots of one (model, period) -- of two at Lmax = 8,
// of at most 64 / (4 Lmax) + 2 -- and walk the layer recursion together: a perturbation moves a layer's value by 2^-14
// at most and with it no lane across a branch (trigonometric or hyperbolic per layer) the others do not take, except
// at a crossing.  Each lane runs two recursions at one perturbed entry and writes one K.  The models a workgroup's
// lanes belong to (255 / (nper 4 Lmax) + 2 at most, 2 KiB / nper + 64 Lmax bytes) are rounded to real*4 once and kept
// in LDS as doubles: a lane reads every layer 2 times per recursion, and the perturbed accessor (SensLay) is a compare
// and a select on the value read.  No scratch: no array is indexed at run time.
#include <hip/hip_runtime.h>
#include "sens_core.h"
#include "sens_launch.h"

namespace bh {

constexpr int SENS_T = 256;

template <int IWAVE>
__global__ __launch_bounds__(SENS_T) void sens_root_kernel(SensArgs A)
{
    const long g = (long)blockIdx.x * SENS_T + threadIdx.x;
    if (g >= (long)A.B * A.nper) return;
    const long b = g / A.nper;
    const int k = (int)(g - b * A.nper);
    const int nl = A.nlay[b];
    const double nan = __builtin_nan("");
    double c = nan, fc = nan, dcdt = nan;
    // the model is read only where the flag and the depth say that it is one (ell_kernel)
    if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax) {
        const long m = b * A.mstride;
        const SensModelLay lay{A.h + m, A.vp + m, A.vs + m, A.rho + m};
        if (sens_model_ok(0, nl, A.Lmax, A.vs[m])) {
            double c1, fc1, dcdt1;
            if (sens_root<IWAVE>(lay, nl, A.periods[k], A.c[b * A.c_stride + k], sens_steps(), c1, fc1, dcdt1)) {
                c = c1; fc = fc1; dcdt = dcdt1;
            }
        }
    }
    A.c_out[g] = c;
    A.fc[g] = fc;
    A.dc_dT[g] = dcdt;
}

extern __shared__ __attribute__((aligned(16))) double sens_lds[];

template <int IWAVE>
__global__ __launch_bounds__(SENS_T) void sens_kernel(SensArgs A)
{
    const int nslot = 4 * A.Lmax;
    const long per_model = (long)A.nper * nslot;
    const long total = (long)A.B * per_model;
    const long g0 = (long)blockIdx.x * SENS_T;
    const long b0 = g0 / per_model;
    long b1 = (g0 + SENS_T - 1) / per_model;
    if (b1 > A.B - 1) b1 = A.B - 1;
    // the block's models, [h | vp | vs | rho] of Lmax real*4 values each; 0 behind a model's last layer and for a row
    // that is no model of this batch
    const int nload = (int)(b1 - b0 + 1) * nslot;
    for (int j = threadIdx.x; j < nload; j += SENS_T) {
        const int m = j / nslot, s = j - m * nslot;
        const int kind = s / A.Lmax, i = s - kind * A.Lmax;
        const long b = b0 + m;
        const int nl = A.nlay[b];
        double v = 0.0;
        if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax && i < nl) {
            const double *row = kind == SENS_H ? A.h : kind == SENS_VP ? A.vp : kind == SENS_VS ? A.vs : A.rho;
            v = (double)(float)row[b * A.mstride + i];
        }
        sens_lds[j] = v;
    }
    __syncthreads();
    const long g = g0 + threadIdx.x;
    if (g >= total) return;
    const long pk = g / nslot;                       // (model, period)
    const int s = (int)(g - pk * nslot);
    const int kind = s / A.Lmax, idx = s - kind * A.Lmax;
    const long b = pk / A.nper;
    const int k = (int)(pk - b * A.nper);
    const double c = A.c_out[pk];
    double r;
    if (c != c) {
        r = __builtin_nan("");                       // no value: the whole (model, period)
    } else {
        const int nl = A.nlay[b];                    // 2 .. Lmax: sens_root_kernel wrote a c
        r = 0.0;                                     // padding layers, the half-space's thickness
        if (idx < nl && !(kind == SENS_H && idx == nl - 1)) {
            const SensRows lay{sens_lds + (b - b0) * nslot, A.Lmax};
            r = sens_slot<IWAVE>(lay, nl, A.periods[k], c, A.fc[pk], kind, idx, sens_steps());
        }
    }
    A.K[g] = r;
}

static size_t sens_lds_bytes(const SensArgs &A)
{
    const long per_model = (long)A.nper * 4 * A.Lmax;
    return (size_t)((SENS_T - 1) / per_model + 2) * 4 * A.Lmax * sizeof(double);
}

bool sens_fits(const SensArgs &A)
{
    const long n = (long)A.B * A.nper * 4 * A.Lmax;
    return (n + SENS_T - 1) / SENS_T <= 0x7fffffffL;
}

hipError_t launch_sens(const SensArgs &A, hipStream_t stream)
{
    const long n1 = (long)A.B * A.nper, n2 = n1 * 4 * A.Lmax;
    const dim3 g1((unsigned)((n1 + SENS_T - 1) / SENS_T)), g2((unsigned)((n2 + SENS_T - 1) / SENS_T));
    const size_t lds = sens_lds_bytes(A);
    if (A.iwave == 2) {
        hipLaunchKernelGGL(sens_root_kernel<2>, g1, dim3(SENS_T), 0, stream, A);
        hipLaunchKernelGGL(sens_kernel<2>, g2, dim3(SENS_T), lds, stream, A);
    } else {
        hipLaunchKernelGGL(sens_root_kernel<1>, g1, dim3(SENS_T), 0, stream, A);
        hipLaunchKernelGGL(sens_kernel<1>, g2, dim3(SENS_T), lds, stream, A);
    }
    return hipGetLastError();
}

}  // namespace bh
