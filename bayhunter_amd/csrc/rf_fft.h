// rf_fft.h -- phase 4's transform of the buffers of one workgroup, device code only: the one function that rf_kernel
// (kernels.hip) and the kernel of bh_selftest_rf_transform (rf_probe.hip) both call.  Its butterflies, plan and swizzle
// are rf_core.h's, which the host replay (rf_host.h: rf_host_fft) runs too.
#pragma once
#include "kernels.h"
#include "rf_core.h"

namespace bh {

// bit reversal (+ 1/sqrt(n)) and the butterfly passes (rf_core.h: one radix-2 stage when log2 n is odd, radix-4 passes
// of two stages each for the rest) of Mb buffers in LDS; all threads of the group
__device__ __forceinline__ void rf_block_fft(double *S, int per_model, int Mb, int n, const RfLaunch &P,
                                             const double *tw, int tid)
{
#if !(defined(BH_RF_EXP) && BH_RF_EXP == 1)
    for (int idx = tid; idx < Mb * n; idx += RF_T) {
        int m = idx / n, i = idx - m * n;
        rf_fft_bitrev_scale(S + (long)m * per_model, n, P.log2n, P.sc, i);
    }
    __syncthreads();
#endif
#if defined(BH_RF_EXP) && BH_RF_EXP == 2
    return;
#endif
    if (rf_fft_radix2_first(P.log2n)) {              // odd log2 n: one radix-2 stage, the rest in pairs
        for (int idx = tid; idx < Mb * (n / 2); idx += RF_T) {
            int m = idx / (n / 2), bf = idx - m * (n / 2);
            rf_fft_butterfly(S + (long)m * per_model, tw, 1, bf);
        }
        __syncthreads();
    }
    for (int l = rf_fft_radix4_first(P.log2n); 4 * l <= n; l <<= 2) {
        for (int idx = tid; idx < Mb * (n / 4); idx += RF_T) {
            int m = idx / (n / 4), bf = idx - m * (n / 4);
            rf_fft_butterfly4(S + (long)m * per_model, tw, l, bf);
        }
        __syncthreads();
    }
}

}  // namespace bh
