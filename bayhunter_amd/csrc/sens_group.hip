// sens_group.hip -- sens_group_root_kernel and sens_group_kernel: the sensitivity kernels dU/dm of the fundamental-mode
// group velocity for a batch of models (sens_group_core.h).  The two kernels of sensitivity.hip with three roots and
// three slot evaluations where those have one.
//
// sens_group_root_kernel, one lane per (model, period): lane g is period g % nper of model g / nper.  It polishes the
// stored root as sens_root_kernel does, finds the roots at T (1 +- r_g) from its tangent, and writes c, U and dU/dT
// and six doubles of workspace -- F_c, c+, F_c+, c-, F_c-, dc/dT, each a plane of B nper values so that the lanes of a
// wave write neighbours.  Where one of the three roots has no value every one of the nine is NaN.
//
// sens_group_kernel, one lane per (model, period, slot) with the slot the fastest index, sens_kernel's layout and its
// real*4-rounded model image in dynamic LDS.  Each lane runs sens_slot at T, T+ and T- (six recursions at one perturbed
// entry) and the combine, and writes one K^U -- and the phase kernel at T, which it has anyway, when asked.  No
// scratch: no array is indexed at run time; no static LDS.
#include <hip/hip_runtime.h>
#include "sens_group_core.h"
#include "sens_group_launch.h"

namespace bh {

constexpr int SENS_GROUP_T = 256;

template <int IWAVE>
__global__ __launch_bounds__(SENS_GROUP_T) void sens_group_root_kernel(SensGroupArgs A)
{
    const long n = (long)A.B * A.nper;
    const long g = (long)blockIdx.x * SENS_GROUP_T + threadIdx.x;
    if (g >= n) return;
    const long b = g / A.nper;
    const int k = (int)(g - b * A.nper);
    const int nl = A.nlay[b];
    const double nan = __builtin_nan("");
    SensGroupRoots R;
    R.c = R.fc = R.dcdt = R.cp = R.fcp = R.cm = R.fcm = R.U = R.dU_dT = nan;
    // the model is read only where the flag and the depth say that it is one (sens_root_kernel)
    if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax) {
        const long m = b * A.mstride;
        const SensModelLay lay{A.h + m, A.vp + m, A.vs + m, A.rho + m};
        if (sens_model_ok(0, nl, A.Lmax, A.vs[m])) {
            SensGroupRoots R1;
            if (sens_group_roots<IWAVE>(lay, nl, A.periods[k], A.c[b * A.c_stride + k], sens_steps(), sens_group_steps(), R1))
                R = R1;
        }
    }
    A.c_out[g] = R.c;
    A.U[g] = R.U;
    A.dU_dT[g] = R.dU_dT;
    A.ws[g] = R.fc;
    A.ws[n + g] = R.cp;
    A.ws[2 * n + g] = R.fcp;
    A.ws[3 * n + g] = R.cm;
    A.ws[4 * n + g] = R.fcm;
    A.ws[5 * n + g] = R.dcdt;
}

extern __shared__ __attribute__((aligned(16))) double sens_group_lds[];

template <int IWAVE>
__global__ __launch_bounds__(SENS_GROUP_T) void sens_group_kernel(SensGroupArgs A)
{
    const int nslot = 4 * A.Lmax;
    const long per_model = (long)A.nper * nslot;
    const long total = (long)A.B * per_model;
    const long g0 = (long)blockIdx.x * SENS_GROUP_T;
    const long b0 = g0 / per_model;
    long b1 = (g0 + SENS_GROUP_T - 1) / per_model;
    if (b1 > A.B - 1) b1 = A.B - 1;
    // the block's models, [h | vp | vs | rho] of Lmax real*4 values each; 0 behind a model's last layer and for a row
    // that is no model of this batch (sens_kernel)
    const int nload = (int)(b1 - b0 + 1) * nslot;
    for (int j = threadIdx.x; j < nload; j += SENS_GROUP_T) {
        const int m = j / nslot, s = j - m * nslot;
        const int kind = s / A.Lmax, i = s - kind * A.Lmax;
        const long b = b0 + m;
        const int nl = A.nlay[b];
        double v = 0.0;
        if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax && i < nl) {
            const double *row = kind == SENS_H ? A.h : kind == SENS_VP ? A.vp : kind == SENS_VS ? A.vs : A.rho;
            v = (double)(float)row[b * A.mstride + i];
        }
        sens_group_lds[j] = v;
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
        const int nl = A.nlay[b];                    // 2 .. Lmax: sens_group_root_kernel wrote a c
        r = r0 = 0.0;                                // padding layers, the half-space's thickness
        if (idx < nl && !(kind == SENS_H && idx == nl - 1)) {
            const SensRows lay{sens_group_lds + (b - b0) * nslot, A.Lmax};
            r = sens_group_slot<IWAVE>(lay, nl, A.periods[k], sens_group_steps().rg, c, A.ws[pk], A.ws[n + pk], A.ws[2 * n + pk],
                                       A.ws[3 * n + pk], A.ws[4 * n + pk], A.U[pk], kind, idx, sens_steps(), r0);
        }
    }
    A.K[g] = r;
    if (A.K_phase) A.K_phase[g] = r0;
}

static size_t sens_group_lds_bytes(const SensGroupArgs &A)
{
    const long per_model = (long)A.nper * 4 * A.Lmax;
    return (size_t)((SENS_GROUP_T - 1) / per_model + 2) * 4 * A.Lmax * sizeof(double);
}

bool sens_group_fits(const SensGroupArgs &A)
{
    const long n = (long)A.B * A.nper * 4 * A.Lmax;
    return (n + SENS_GROUP_T - 1) / SENS_GROUP_T <= 0x7fffffffL;
}

hipError_t launch_sens_group(const SensGroupArgs &A, hipStream_t stream)
{
    const long n1 = (long)A.B * A.nper, n2 = n1 * 4 * A.Lmax;
    const dim3 g1((unsigned)((n1 + SENS_GROUP_T - 1) / SENS_GROUP_T)), g2((unsigned)((n2 + SENS_GROUP_T - 1) / SENS_GROUP_T));
    const size_t lds = sens_group_lds_bytes(A);
    if (A.iwave == 2) {
        hipLaunchKernelGGL(sens_group_root_kernel<2>, g1, dim3(SENS_GROUP_T), 0, stream, A);
        hipLaunchKernelGGL(sens_group_kernel<2>, g2, dim3(SENS_GROUP_T), lds, stream, A);
    } else {
        hipLaunchKernelGGL(sens_group_root_kernel<1>, g1, dim3(SENS_GROUP_T), 0, stream, A);
        hipLaunchKernelGGL(sens_group_kernel<1>, g2, dim3(SENS_GROUP_T), lds, stream, A);
    }
    return hipGetLastError();
}

}  // namespace bh
