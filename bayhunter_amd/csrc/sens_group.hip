// sens_group.hip -- sens_group_root_kernel and sens_group_kernel: the sensitivity kernels dU/dm of the fundamental-mode
// group velocity for a batch of models (sens_group_core.h).  The pass of sens_pass.h with three roots and three slot
// evaluations where the phase pass has one.
//
// sens_group_root_kernel polishes the stored root as sens_root_kernel does, finds the roots at T (1 +- r_g) from its
// tangent, and writes c, U and dU/dT and six doubles of workspace -- F_c, c+, F_c+, c-, F_c-, dc/dT, each a plane of
// B nper values so that the lanes of a wave write neighbours.  Where one of the three roots has no value every one of
// the nine is NaN.
//
// sens_group_kernel's lanes run sens_slot at T, T+ and T- (six recursions at one perturbed entry) and the combine, and
// write one K^U -- and the phase kernel at T, which they have anyway, when asked.
#include <hip/hip_runtime.h>
#include "sens_group_core.h"
#include "sens_pass.h"

namespace bh {

template <int IWAVE>
__global__ __launch_bounds__(SENS_PASS_T) void sens_group_root_kernel(SensGroupArgs A)
{
    const long n = (long)A.B * A.nper;
    const long g = (long)blockIdx.x * SENS_PASS_T + threadIdx.x;
    if (g >= n) return;
    const double nan = __builtin_nan("");
    SensGroupRoots R;
    R.c = R.fc = R.dcdt = R.cp = R.fcp = R.cm = R.fcm = R.U = R.dU_dT = nan;
    sens_pass_root_lane(A, g, [&](long b, int k, int nl, const SensModelLay &lay) {
        SensGroupRoots R1;
        if (sens_group_roots<IWAVE>(lay, nl, A.periods[k], A.c[b * A.c_stride + k], sens_steps(), sens_group_steps(), R1))
            R = R1;
    });
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
__global__ __launch_bounds__(SENS_PASS_T) void sens_group_kernel(SensGroupArgs A)
{
    sens_pass_slot_lane(A, A.K_phase, sens_group_lds,
                        [&](const SensRows &lay, int nl, int k, long pk, double c, int kind, int idx, double &r0) {
                            const long n = (long)A.B * A.nper;
                            return sens_group_slot<IWAVE>(lay, nl, A.periods[k], sens_group_steps().rg, c, A.ws[pk], A.ws[n + pk],
                                                          A.ws[2 * n + pk], A.ws[3 * n + pk], A.ws[4 * n + pk], A.U[pk], kind, idx,
                                                          sens_steps(), r0);
                        });
}

hipError_t launch_sens_group(const SensGroupArgs &A, hipStream_t stream)
{
    return A.iwave == 2 ? sens_pass_launch(sens_group_root_kernel<2>, sens_group_kernel<2>, A, stream)
                        : sens_pass_launch(sens_group_root_kernel<1>, sens_group_kernel<1>, A, stream);
}

}  // namespace bh
