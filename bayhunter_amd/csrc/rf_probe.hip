// rf_probe.hip -- the kernel of bh_selftest_rf_transform: phase 4 of rf_kernel alone, on spectra the caller gives.
//
// A translation unit of its own, so that no other kernel's registers or listing depend on it.  The workgroup is
// rf_kernel's: RF_T threads, M buffers in LDS at the pitch rf_layout(Lmax, nsamp).per_model (+ the 4 nfreq doubles of
// the trace form's two spectra behind each block when paired), the twiddle table of get_twiddles (rf_capi.hip), and from
// "P4" on the statements of rf_kernel with the same functions: rf_xst, rf_fft_hermitian, rf_block_fft (rf_fft.h),
// rf_fft_pair_entry.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rf_core.h"
#include "rf_fft.h"

namespace bh {

// spec [B][paired ? 2 : 1][nfreq][2], out [B][paired ? 2 : 1][nout].  P: nsamp, nfreq, log2n, sc, qn, nout, Lmax, M.
__global__ __launch_bounds__(RF_T) void rf_probe_kernel(RfLaunch P, int B, int paired, const double *BH_RESTRICT spec,
                                                        const double *BH_RESTRICT tw, double *BH_RESTRICT out)
{
    extern __shared__ double S[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * P.M;
    const int Mb = min(P.M, B - b0);
    const RfLayout lo = rf_layout(P.Lmax, P.nsamp);
    const int n = P.nsamp, nf = P.nfreq, nch = paired ? 2 : 1;
    const int pm = lo.per_model + (paired ? 4 * nf : 0);    // paired: [spec_r | spec_z] behind the block

    // what phase 3 leaves: the half spectrum in the (swizzled) buffer; paired: the two spectra behind the block, and
    // the first of them in the buffer, which the first transform then uses up as rf_kernel<true>'s uses up the RF's
    for (int idx = tid; idx < Mb * nf; idx += RF_T) {
        int m = idx / nf, j = idx - m * nf;
        double *Sm = S + (long)m * pm;
        const double *sp = spec + ((long)(b0 + m) * nch * nf + j) * 2;
        rf_xst(Sm, j, ld_cd(sp));
        if (paired) {
            st_cd(Sm + lo.per_model + 2 * j, ld_cd(sp));
            st_cd(Sm + lo.per_model + 2 * nf + 2 * j, ld_cd(sp + 2 * nf));
        }
    }
    __syncthreads();
    // P4: inverse FFT in LDS (iftr, greens.cpp:136-158)
    const int nh = n / 2 - 1;
    for (int idx = tid; idx < Mb * nh; idx += RF_T) {
        int m = idx / nh, i = n / 2 + 1 + (idx - m * nh);
        rf_fft_hermitian(S + (long)m * pm, n, i);
    }
    __syncthreads();
    rf_block_fft(S, pm, Mb, n, P, tw, tid);
    for (int idx = tid; idx < Mb * P.nout; idx += RF_T) {
        int m = idx / P.nout, i = idx - m * P.nout;
        out[((long)(b0 + m) * nch) * P.nout + i] = P.qn * S[(long)m * pm + 2 * rf_swz(i)];
    }
    if (paired) {   // iftr2 (greens.cpp:161-194): one FFT of cx = first + i * second; both rows are written again
        __syncthreads();
        for (int idx = tid; idx < Mb * n; idx += RF_T) {
            int m = idx / n, i = idx - m * n;
            double *Sm = S + (long)m * pm;
            rf_xst(Sm, i, rf_fft_pair_entry(Sm + lo.per_model, Sm + lo.per_model + 2 * nf, n, i));
        }
        __syncthreads();
        rf_block_fft(S, pm, Mb, n, P, tw, tid);
        for (int idx = tid; idx < Mb * P.nout; idx += RF_T) {     // (the thread that wrote the row's entry i above)
            int m = idx / P.nout, i = idx - m * P.nout;
            const double *Sm = S + (long)m * pm;
            out[((long)(b0 + m) * 2) * P.nout + i] = P.qn * Sm[2 * rf_swz(i)];
            out[((long)(b0 + m) * 2 + 1) * P.nout + i] = P.qn * Sm[2 * rf_swz(i) + 1];
        }
    }
}

hipError_t launch_rf_probe(const RfLaunch &P, int B, int paired, const double *spec, const double *tw, double *out,
                           hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    const size_t lds = rf_lds_bytes(P.Lmax, P.nsamp, P.M, paired != 0);
    if (lds > 48 * 1024) {      // per device, as ensure_dyn_lds (kernels.hip) does it
        static size_t lds_set[16] = {0};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        dev &= 15;
        if (lds > lds_set[dev]) {
            e = hipFuncSetAttribute((const void *)rf_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            lds_set[dev] = lds;
        }
    }
    dim3 grid((B + P.M - 1) / P.M);
    hipLaunchKernelGGL(rf_probe_kernel, grid, dim3(RF_T), lds, stream, P, B, paired ? 1 : 0, spec, tw, out);
    return hipGetLastError();
}

}  // namespace bh
