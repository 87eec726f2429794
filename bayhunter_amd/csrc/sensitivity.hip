// sensitivity.hip -- sens_root_kernel and sens_kernel: the sensitivity kernels dc/dm of the fundamental-mode phase
// velocity for a batch of models (sens_core.h), the first of the three passes of sens_pass.h.
//
// sens_root_kernel writes c, F_c and dc/dT: up to 3 SENS_NEWTON + 4 recursions per lane.  sens_kernel's lanes run two
// recursions at one perturbed entry each.
#include <hip/hip_runtime.h>
#include "sens_pass.h"

namespace bh {

template <int IWAVE>
__global__ __launch_bounds__(SENS_PASS_T) void sens_root_kernel(SensArgs A)
{
    const long g = (long)blockIdx.x * SENS_PASS_T + threadIdx.x;
    if (g >= (long)A.B * A.nper) return;
    const double nan = __builtin_nan("");
    double c = nan, fc = nan, dcdt = nan;
    sens_pass_root_lane(A, g, [&](long b, int k, int nl, const SensModelLay &lay) {
        double c1, fc1, dcdt1;
        if (sens_root<IWAVE>(lay, nl, A.periods[k], A.c[b * A.c_stride + k], sens_steps(), c1, fc1, dcdt1)) {
            c = c1; fc = fc1; dcdt = dcdt1;
        }
    });
    A.c_out[g] = c;
    A.fc[g] = fc;
    A.dc_dT[g] = dcdt;
}

extern __shared__ __attribute__((aligned(16))) double sens_lds[];

template <int IWAVE>
__global__ __launch_bounds__(SENS_PASS_T) void sens_kernel(SensArgs A)
{
    sens_pass_slot_lane(A, nullptr, sens_lds,
                        [&](const SensRows &lay, int nl, int k, long pk, double c, int kind, int idx, double &) {
                            return sens_slot<IWAVE>(lay, nl, A.periods[k], c, A.fc[pk], kind, idx, sens_steps());
                        });
}

hipError_t launch_sens(const SensArgs &A, hipStream_t stream)
{
    return A.iwave == 2 ? sens_pass_launch(sens_root_kernel<2>, sens_kernel<2>, A, stream)
                        : sens_pass_launch(sens_root_kernel<1>, sens_kernel<1>, A, stream);
}

}  // namespace bh
