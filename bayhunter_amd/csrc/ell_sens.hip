// ell_sens.hip -- ell_sens_root_kernel and ell_sens_kernel: the sensitivity kernels d(H/V)/dm of the fundamental
// Rayleigh mode's ellipticity for a batch of models (ell_sens_core.h).  The two kernels of sensitivity.hip with passes
// that return the ratio G beside the period equation F.
//
// ell_sens_root_kernel, one lane per (model, period): lane g is period g % nper of model g / nper.  It polishes the
// stored root as sens_root_kernel does, with the layers read where they lie, and writes c, E and dE/dT and three
// doubles of workspace -- F_c, G_c and the sign E, dE/dT and K are multiplied by -- each a plane of B nper values so
// that the lanes of a wave write neighbours.  Where the (model, period) has no value every one of the six is NaN.
//
// ell_sens_kernel, one lane per (model, period, slot) with the slot the fastest index, sens_kernel's layout and its
// real*4-rounded model image in dynamic LDS (255 / (nper 4 Lmax) + 2 models of 4 Lmax doubles at most).  Each lane runs
// two recursions at one perturbed entry, as sens_kernel's lanes do, takes F and G from each, and writes one K^E -- and
// the phase kernel, which it has anyway, when asked.  No scratch: no array is indexed at run time; no static LDS.
//
// 256 lanes per workgroup, as in sensitivity.hip: the LDS image is 2 KiB / nper + 64 Lmax bytes, never the limit; the
// kernels are bound by their registers (DESIGN.md section 4.1g has the counts), and four waves per workgroup put one
// on each SIMD whatever the number of workgroups a compute unit holds.
#include <hip/hip_runtime.h>
#include "ell_sens_core.h"
#include "ell_sens_launch.h"

namespace bh {

constexpr int ELL_SENS_T = 256;

__global__ __launch_bounds__(ELL_SENS_T) void ell_sens_root_kernel(EllSensArgs A)
{
    const long n = (long)A.B * A.nper;
    const long g = (long)blockIdx.x * ELL_SENS_T + threadIdx.x;
    if (g >= n) return;
    const long b = g / A.nper;
    const int k = (int)(g - b * A.nper);
    const int nl = A.nlay[b];
    const double nan = __builtin_nan("");
    double c = nan, E = nan, dEdT = nan, fc = nan, gc = nan, sgn = nan;
    // the model is read only where the flag and the depth say that it is one (sens_root_kernel)
    if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax) {
        const long m = b * A.mstride;
        const SensModelLay lay{A.h + m, A.vp + m, A.vs + m, A.rho + m};
        if (sens_model_ok(0, nl, A.Lmax, A.vs[m])) {
            EllSensRoot R;
            if (ell_sens_root<ELL_FORM_TZ>(lay, nl, A.periods[k], A.c[b * A.c_stride + k], ell_sens_steps(), R)) {
                sgn = A.absolute ? R.sgn : 1.0;
                c = R.c; E = sgn * R.E; dEdT = sgn * R.dE_dT; fc = R.fc; gc = R.gc;
            }
        }
    }
    A.c_out[g] = c;
    A.E[g] = E;
    A.dE_dT[g] = dEdT;
    A.ws[g] = fc;
    A.ws[n + g] = gc;
    A.ws[2 * n + g] = sgn;
}

extern __shared__ __attribute__((aligned(16))) double ell_sens_lds[];

__global__ __launch_bounds__(ELL_SENS_T) void ell_sens_kernel(EllSensArgs A)
{
    const int nslot = 4 * A.Lmax;
    const long per_model = (long)A.nper * nslot;
    const long total = (long)A.B * per_model;
    const long g0 = (long)blockIdx.x * ELL_SENS_T;
    const long b0 = g0 / per_model;
    long b1 = (g0 + ELL_SENS_T - 1) / per_model;
    if (b1 > A.B - 1) b1 = A.B - 1;
    // the block's models, [h | vp | vs | rho] of Lmax real*4 values each; 0 behind a model's last layer and for a row
    // that is no model of this batch (sens_kernel)
    const int nload = (int)(b1 - b0 + 1) * nslot;
    for (int j = threadIdx.x; j < nload; j += ELL_SENS_T) {
        const int m = j / nslot, s = j - m * nslot;
        const int kind = s / A.Lmax, i = s - kind * A.Lmax;
        const long b = b0 + m;
        const int nl = A.nlay[b];
        double v = 0.0;
        if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax && i < nl) {
            const double *row = kind == SENS_H ? A.h : kind == SENS_VP ? A.vp : kind == SENS_VS ? A.vs : A.rho;
            v = (double)(float)row[b * A.mstride + i];
        }
        ell_sens_lds[j] = v;
    }
    __syncthreads();
    const long g = g0 + threadIdx.x;
    if (g >= total) return;
    const long pk = g / nslot;                       // (model, period)
    const int s = (int)(g - pk * nslot);
    const int kind = s / A.Lmax, idx = s - kind * A.Lmax;
    const long b = pk / A.nper;
    const int k = (int)(pk - b * A.nper);
    const long n = (long)A.B * A.nper;
    const double c = A.c_out[pk];
    double r, r0;
    if (c != c) {
        r = r0 = __builtin_nan("");                  // no value: the whole (model, period)
    } else {
        const int nl = A.nlay[b];                    // 2 .. Lmax: ell_sens_root_kernel wrote a c
        r = r0 = 0.0;                                // padding layers, the half-space's thickness
        if (idx < nl && !(kind == SENS_H && idx == nl - 1)) {
            const SensRows lay{ell_sens_lds + (b - b0) * nslot, A.Lmax};
            r = A.ws[2 * n + pk] * ell_sens_slot<ELL_FORM_TZ>(lay, nl, A.periods[k], c, A.ws[pk], A.ws[n + pk], kind, idx,
                                                             ell_sens_steps(), r0);
        }
    }
    A.K[g] = r;
    if (A.K_phase) A.K_phase[g] = r0;
}

static size_t ell_sens_lds_bytes(const EllSensArgs &A)
{
    const long per_model = (long)A.nper * 4 * A.Lmax;
    return (size_t)((ELL_SENS_T - 1) / per_model + 2) * 4 * A.Lmax * sizeof(double);
}

bool ell_sens_fits(const EllSensArgs &A)
{
    const long n = (long)A.B * A.nper * 4 * A.Lmax;
    return (n + ELL_SENS_T - 1) / ELL_SENS_T <= 0x7fffffffL;
}

hipError_t launch_ell_sens(const EllSensArgs &A, hipStream_t stream)
{
    const long n1 = (long)A.B * A.nper, n2 = n1 * 4 * A.Lmax;
    const dim3 g1((unsigned)((n1 + ELL_SENS_T - 1) / ELL_SENS_T)), g2((unsigned)((n2 + ELL_SENS_T - 1) / ELL_SENS_T));
    hipLaunchKernelGGL(ell_sens_root_kernel, g1, dim3(ELL_SENS_T), 0, stream, A);
    hipLaunchKernelGGL(ell_sens_kernel, g2, dim3(ELL_SENS_T), ell_sens_lds_bytes(A), stream, A);
    return hipGetLastError();
}

}  // namespace bh
