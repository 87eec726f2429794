// math_probe.hip -- the kernel of bh_selftest_math: one primitive of math_probe.h per thread.
//
// A translation unit of its own, so that no other kernel's registers or listing depend on it.
#include <hip/hip_runtime.h>
#include "math_probe.h"

namespace bh {

constexpr int MP_T = 256;

// Thread i handles element i: wave w holds elements 64 w .. 64 w + 63 (math_probe.h).  `op` is a kernel argument, so the
// switch is a scalar branch and the primitive runs under the exec mask of the `i < n` guard alone.
__global__ __launch_bounds__(MP_T) void math_probe_kernel(int op, long n, const double *BH_RESTRICT in,
                                                          double *BH_RESTRICT out)
{
    const long i = (long)blockIdx.x * MP_T + threadIdx.x;
    if (i < n) {
        double x[MP_IN], y[MP_OUT];
        for (int k = 0; k < MP_IN; k++) x[k] = in[MP_IN * i + k];
        math_probe_apply(op, x, y);
        for (int k = 0; k < MP_OUT; k++) out[MP_OUT * i + k] = y[k];
    }
}

hipError_t launch_math_probe(int op, long n, const double *in, double *out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const long blocks = (n + MP_T - 1) / MP_T;
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)blocks), dim3(MP_T), 0, stream, op, n, in, out);
    return hipGetLastError();
}

}  // namespace bh
