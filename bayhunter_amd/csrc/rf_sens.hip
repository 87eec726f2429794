// rf_sens.hip -- rf_sens_kernel: sensitivity kernels dRF(t)/dm of the receiver function (rf_sens_core.h).
//
// A workgroup takes one model and a run of its 4 nlay - 1 slots.  Every (slot, sign) is a variant: a copy of the
// model's four rows with one entry times 1 +- r, staged in LDS behind an LDS block laid out like a model's block in
// rf_kernel (rf_layout), on which the phases of rf_core.h and rf_fft.h run exactly as rf_kernel runs them on global
// rows -- rf_phase1_layer, rf_phase2_interface, rf_phase3_task_at, the Hermitian fill and rf_block_fft, with
// rf_kernel's barriers between them.  Behind the transform the difference of a slot's two buffers is written to K.
// The perturbed traces never leave LDS and no expanded batch of models exists anywhere.
//
// PAIRED: `pairs` (+, -) pairs per workgroup, 2 pairs blocks (rf_sens_pairs: as many as 40 KiB hold, four workgroups
// per CU).  Sequential form (one block; the lengths at which a pair no longer fits that budget): the + and the - variant
// of the workgroup's one slot run one after the other on the same block, the first trace waits in registers (sixteen
// samples per thread at the longest transform).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "rf_fft.h"
#include "host_common.h"
#include "rf_sens_core.h"

namespace bh {

constexpr int RF_SENS_KEEP = 4096 / RF_T;       // samples per thread the sequential form keeps: the longest transform

// Phases 1 to 4 on the nvar variants of the workgroup: variant v is slot slot0 + v / per_slot, sign (v % per_slot) or
// `pass` (sequential form: per_slot = 1).  Leaves the transformed buffers (before qn) in the blocks.
__device__ __forceinline__ void rf_sens_phases(double *S, const RfSensArgs &A, const RfLayout &lo, int pitch, long b, int nl,
                                               int slot0, int nvar, int per_slot, int pass, int tid)
{
    const RfLaunch &P = A.P;
    const int L = P.Lmax, n = P.nsamp;
    const double *gh = A.h + b * A.mstride, *gvp = A.vp + b * A.mstride, *gvs = A.vs + b * A.mstride,
                 *grho = A.rho + b * A.mstride;
    // the perturbed copies of the four rows, behind each variant's block
    for (int idx = tid; idx < nvar * 4 * L; idx += RF_T) {
        const int v = idx / (4 * L), e = idx - v * 4 * L;
        int kind, i;
        rf_sens_slot(nl, slot0 + v / per_slot, &kind, &i);
        const double r = rf_sens_step_of(A.st, kind);
        const int sign = per_slot == 2 ? (v & 1) : pass;
        S[(long)v * pitch + lo.per_model + e] = rf_sens_staged(gh, gvp, gvs, grho, L, nl, e, kind, i, sign ? 1.0 - r : 1.0 + r);
    }
    __syncthreads();
    // P1: flatten layers
    for (int idx = tid; idx < nvar * L; idx += RF_T) {
        const int v = idx / L, i = idx - v * L;
        double *Sv = S + (long)v * pitch;
        const double *rows = Sv + lo.per_model;
        if (i < nl)
            rf_phase1_layer(Sv, lo, nl, i, rows, rows + L, rows + 2 * L, rows + 3 * L, A.qp ? A.qp + b * L : nullptr,
                            A.qs ? A.qs + b * L : nullptr, 0);
    }
    __syncthreads();
    // P2: interface coefficients (+ per-variant scalars on interface 0; the rotation is the perturbed top layer's)
    for (int idx = tid; idx < nvar * L; idx += RF_T) {
        const int v = idx / L, i = idx - v * L;
        double *Sv = S + (long)v * pitch;
        const double *rows = Sv + lo.per_model;
        if (i < nl) rf_phase2_interface(Sv, lo, P, nl, i, rows[L], rows[2 * L]);
    }
    __syncthreads();
    // P3: (variant, frequency) tasks, variant-major
    const int ntask = nvar * P.nact;
    for (int task = tid; task < ntask; task += RF_T) {
        const int v = task / P.nact, j = task - v * P.nact;
        double *Sv = S + (long)v * pitch;
        const cd crf = rf_phase3_task_at<false>(Sv, lo, P, nl, j, rf_freq_load(A.ftab, j), nullptr, nullptr, A.ftab);
        rf_xst(Sv, j, crf);
    }
    const int nzero = P.nfreq - P.nact;
    for (int idx = tid; idx < nvar * nzero; idx += RF_T) {
        const int v = idx / nzero, j = P.nact + (idx - v * nzero);
        rf_xst(S + (long)v * pitch, j, mk(0., 0.));
    }
    __syncthreads();
    // P4: inverse FFT in LDS
    const int nh = n / 2 - 1;
    for (int idx = tid; idx < nvar * nh; idx += RF_T) {
        const int v = idx / nh, i = n / 2 + 1 + (idx - v * nh);
        rf_fft_hermitian(S + (long)v * pitch, n, i);
    }
    __syncthreads();
    rf_block_fft(S, pitch, nvar, n, P, A.tw, tid);      // (ends with a barrier)
}

// The cells of model b's K no slot writes: NaN in the layers from nlay on (all of them for nlay outside 1 .. Lmax),
// 0 for the half-space's thickness.
__device__ __forceinline__ void rf_sens_fill(const RfSensArgs &A, long b, int nlay_in, int tid)
{
    const int L = A.P.Lmax, nout = A.P.nout;
    const bool bad = nlay_in < 1 || nlay_in > L;
    double *Kb = A.K + b * A.k_stride;
    for (long idx = tid; idx < (long)nout * 4 * L; idx += RF_T) {
        const int i = (int)(idx % L), kind = (int)((idx / L) & 3);
        if (bad || i >= nlay_in) Kb[idx] = __builtin_nan("");
        else if (kind == SENS_H && i == nlay_in - 1) Kb[idx] = 0.0;
    }
}

template <bool PAIRED>
__global__ __launch_bounds__(RF_T) void rf_sens_kernel(RfSensArgs A)
{
    extern __shared__ double S[];
    const RfLaunch &P = A.P;
    const int tid = threadIdx.x;
    const int L = P.Lmax;
    const int pairs = PAIRED ? A.pairs : 1;
    const int chunks = (4 * L - 1 + pairs - 1) / pairs;
    const long b = blockIdx.x / chunks;
    const int slot0 = (int)(blockIdx.x - b * chunks) * pairs;
    const int nlay_in = A.nlay[b];
    if (slot0 == 0) rf_sens_fill(A, b, nlay_in, tid);
    if (nlay_in < 1 || nlay_in > L) return;
    const int nl = nlay_in;
    const int nslot = min(pairs, rf_sens_nslots(nl) - slot0);
    if (nslot < 1) return;                              // (the whole workgroup: no barrier has been reached)
    const RfLayout lo = rf_layout(L, P.nsamp);
    const int pitch = lo.per_model + 4 * L;             // a block and the variant's four rows behind it
    double *Kb = A.K + b * A.k_stride;

    if (PAIRED) {
        rf_sens_phases(S, A, lo, pitch, b, nl, slot0, 2 * nslot, 2, 0, tid);
        for (int idx = tid; idx < nslot * P.nout; idx += RF_T) {
            const int q = idx / P.nout, t = idx - q * P.nout;
            int kind, i;
            rf_sens_slot(nl, slot0 + q, &kind, &i);
            const double r = rf_sens_step_of(A.st, kind);
            const double v = rf_sens_staged(A.h + b * A.mstride, A.vp + b * A.mstride, A.vs + b * A.mstride,
                                            A.rho + b * A.mstride, L, nl, kind * L + i, -1, -1, 1.0);
            const double *Sp = S + (long)(2 * q) * pitch, *Sm = Sp + pitch;
            Kb[((long)t * 4 + kind) * L + i] = rf_sens_value(P.qn, Sp[2 * rf_swz(t)], Sm[2 * rf_swz(t)], v, r);
        }
    } else {
        double keep[RF_SENS_KEEP];
        rf_sens_phases(S, A, lo, pitch, b, nl, slot0, 1, 1, 0, tid);
#pragma unroll
        for (int k = 0; k < RF_SENS_KEEP; k++) {
            const int t = tid + k * RF_T;
            keep[k] = t < P.nout ? S[2 * rf_swz(t)] : 0.0;
        }
        __syncthreads();                                // the block is staged again
        rf_sens_phases(S, A, lo, pitch, b, nl, slot0, 1, 1, 1, tid);
        int kind, i;
        rf_sens_slot(nl, slot0, &kind, &i);
        const double r = rf_sens_step_of(A.st, kind);
        const double v = rf_sens_staged(A.h + b * A.mstride, A.vp + b * A.mstride, A.vs + b * A.mstride,
                                        A.rho + b * A.mstride, L, nl, kind * L + i, -1, -1, 1.0);
#pragma unroll
        for (int k = 0; k < RF_SENS_KEEP; k++) {
            const int t = tid + k * RF_T;
            if (t < P.nout) Kb[((long)t * 4 + kind) * L + i] = rf_sens_value(P.qn, keep[k], S[2 * rf_swz(t)], v, r);
        }
    }
}

hipError_t launch_rf_sens(const RfSensArgs &A0, hipStream_t stream)
{
    RfSensArgs A = A0;
    A.pairs = rf_sens_pairs(A.P.Lmax, A.P.nsamp);
    const bool paired = A.pairs > 0;
    const int per = paired ? A.pairs : 1;
    const size_t lds = rf_sens_lds_bytes(A.P.Lmax, A.P.nsamp, paired ? 2 * A.pairs : 1);
    if (lds > kLdsLimit) return hipErrorInvalidValue;
    void (*kern)(RfSensArgs) = paired ? rf_sens_kernel<true> : rf_sens_kernel<false>;
    if (lds > 48 * 1024) {      // per device, as ensure_dyn_lds (kernels.hip) does it
        static size_t lds_set[2][16] = {{0}, {0}};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        dev &= 15;
        if (lds > lds_set[paired][dev]) {
            e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            lds_set[paired][dev] = lds;
        }
    }
    const long chunks = (4 * A.P.Lmax - 1 + per - 1) / per;
    hipLaunchKernelGGL(kern, dim3((unsigned)(A.B * chunks)), dim3(RF_T), lds, stream, A);
    return hipGetLastError();
}

}  // namespace bh
