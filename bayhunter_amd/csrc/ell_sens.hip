// ell_sens.hip -- ell_sens_root_kernel and ell_sens_kernel: the sensitivity kernels d(H/V)/dm of the fundamental
// Rayleigh mode's ellipticity for a batch of models (ell_sens_core.h).  The pass of sens_pass.h with recursions that
// return the ratio G beside the period equation F.
//
// ell_sens_root_kernel polishes the stored root as sens_root_kernel does and writes c, E and dE/dT and three doubles
// of workspace -- F_c, G_c and the sign E, dE/dT and K are multiplied by -- each a plane of B nper values so that the
// lanes of a wave write neighbours.  Where the (model, period) has no value every one of the six is NaN.
//
// ell_sens_kernel's lanes run two recursions at one perturbed entry, as sens_kernel's do, take F and G from each, and
// write one K^E -- and the phase kernel, which they have anyway, when asked.
#include <hip/hip_runtime.h>
#include "ell_sens_core.h"
#include "sens_pass.h"

namespace bh {

__global__ __launch_bounds__(SENS_PASS_T) void ell_sens_root_kernel(EllSensArgs A)
{
    const long n = (long)A.B * A.nper;
    const long g = (long)blockIdx.x * SENS_PASS_T + threadIdx.x;
    if (g >= n) return;
    const double nan = __builtin_nan("");
    double c = nan, E = nan, dEdT = nan, fc = nan, gc = nan, sgn = nan;
    sens_pass_root_lane(A, g, [&](long b, int k, int nl, const SensModelLay &lay) {
        EllSensRoot R;
        if (ell_sens_root<ELL_FORM_TZ>(lay, nl, A.periods[k], A.c[b * A.c_stride + k], ell_sens_steps(), R)) {
            sgn = A.absolute ? R.sgn : 1.0;
            c = R.c; E = sgn * R.E; dEdT = sgn * R.dE_dT; fc = R.fc; gc = R.gc;
        }
    });
    A.c_out[g] = c;
    A.E[g] = E;
    A.dE_dT[g] = dEdT;
    A.ws[g] = fc;
    A.ws[n + g] = gc;
    A.ws[2 * n + g] = sgn;
}

extern __shared__ __attribute__((aligned(16))) double ell_sens_lds[];

__global__ __launch_bounds__(SENS_PASS_T) void ell_sens_kernel(EllSensArgs A)
{
    sens_pass_slot_lane(A, A.K_phase, ell_sens_lds,
                        [&](const SensRows &lay, int nl, int k, long pk, double c, int kind, int idx, double &r0) {
                            const long n = (long)A.B * A.nper;
                            return A.ws[2 * n + pk] * ell_sens_slot<ELL_FORM_TZ>(lay, nl, A.periods[k], c, A.ws[pk], A.ws[n + pk],
                                                                                 kind, idx, ell_sens_steps(), r0);
                        });
}

hipError_t launch_ell_sens(const EllSensArgs &A, hipStream_t stream)
{
    return sens_pass_launch(ell_sens_root_kernel, ell_sens_kernel, A, stream);
}

}  // namespace bh
