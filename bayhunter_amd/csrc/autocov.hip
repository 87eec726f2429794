// autocov.hip -- autocovariances of many run-length coded series in one launch (bh_autocov_sets).
//
// What the convergence diagnostics (bayhunter_amd/convergence.py) need beyond the segmented column reduction: per half
// chain and column the autocovariance at lags 0 .. nlags - 1 of the series in which every row is repeated `weight`
// times.  The result is defined exactly in autocov_core.h; the device returns the bits of the host build.
//
//   autocov_block_sums, autocov_scan_sums, autocov_scan_rows
//                        the exclusive prefix sum of the weights over all rows (cum[nrows + 1]): where a row's samples
//                        begin.  Stretches of kScanRows rows: their sums, the sums' prefix by one block, the rows' own.
//   autocov_lengths      n_s = cum[start[s + 1]] - cum[start[s]] per series, for the host
//   autocov_kernel       a block per (series, column, group of lags): tile by tile it expands and centres the series
//                        into the planes of its LDS -- thread i takes rows first + i, first + i + threads, .., the first
//                        row of a tile found by bisection in cum -- and runs autocov_tile over it; at the series' end
//                        it divides by n.
//
// Integer sums and one fixed chain of fused multiply-adds per result: two runs are bit-identical, whatever the grid.
#include <cstring>
#include <string>
#include <vector>
#include "autocov_core.h"
#include "host_common.h"
#include "stats_host.h"

namespace {

using bh::u64;
constexpr int L = bh::kAutocovLags;
constexpr int kScanThreads = 256, kScanPer = 16, kScanRows = kScanThreads * kScanPer;

// Σ of the block's thread values over the threads before this one, and the block's total; s_scan [kScanThreads]
__device__ __forceinline__ long long block_exclusive(long long v, long long *s_scan, long long *total)
{
    const int tid = threadIdx.x;
    s_scan[tid] = v;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const long long add = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const long long inc = s_scan[tid];
    *total = s_scan[kScanThreads - 1];
    __syncthreads();
    return inc - v;
}

__device__ __forceinline__ long long thread_rows(const int *w, long long nrows, long long r0, u64 *bad)
{
    long long s = 0;
    for (int i = 0; i < kScanPer; i++) {
        const long long r = r0 + i;
        if (r < nrows) {
            const int wt = w[r];
            if (wt < 0 && bad) (*bad)++;
            s += wt > 0 ? wt : 0;
        }
    }
    return s;
}

__global__ __launch_bounds__(kScanThreads) void autocov_block_sums(const int *w, long long nrows, long long *bsum, u64 *neg)
{
    __shared__ long long s_scan[kScanThreads];
    u64 bad = 0;
    const long long v = thread_rows(w, nrows, (long long)blockIdx.x * kScanRows + (long long)threadIdx.x * kScanPer, &bad);
    long long total;
    (void)block_exclusive(v, s_scan, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    if (bad) atomicAdd(neg, bad);
}

// one block: bsum[nb] -> its exclusive prefix in place, the total to *end
__global__ __launch_bounds__(kScanThreads) void autocov_scan_sums(long long *bsum, long long nb, long long *end)
{
    __shared__ long long s_scan[kScanThreads];
    long long carry = 0;
    for (long long b0 = 0; b0 < nb; b0 += kScanThreads) {
        const long long b = b0 + threadIdx.x;
        const long long v = b < nb ? bsum[b] : 0;
        long long total;
        const long long ex = block_exclusive(v, s_scan, &total);
        if (b < nb) bsum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *end = carry;
}

__global__ __launch_bounds__(kScanThreads) void autocov_scan_rows(const int *w, long long nrows, const long long *boff,
                                                                  long long *cum)
{
    __shared__ long long s_scan[kScanThreads];
    const long long r0 = (long long)blockIdx.x * kScanRows + (long long)threadIdx.x * kScanPer;
    const long long v = thread_rows(w, nrows, r0, nullptr);
    long long total;
    long long at = boff[blockIdx.x] + block_exclusive(v, s_scan, &total);
    for (int i = 0; i < kScanPer; i++) {
        const long long r = r0 + i;
        if (r < nrows) {
            cum[r] = at;
            const int wt = w[r];
            at += wt > 0 ? wt : 0;
        }
    }
}

__global__ void autocov_lengths(const long long *cum, const long long *start, int nseries, long long *len)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseries) return;
    len[s] = cum ? cum[start[s + 1]] - cum[start[s]] : start[s + 1] - start[s];
}

struct AutocovArgs {
    const double *D; long long stride; int ncols;
    const long long *cum;              // [nrows + 1], or NULL: every weight is 1
    const long long *start;            // [nseries + 1]
    const double *mean;                // [nseries][ncols]
    int nlags, ngroups, group_lags, tile, pitch;
    double *acov;                      // [nseries][ncols][nlags]
};

__global__ __launch_bounds__(bh::kAutocovThreads) void autocov_kernel(AutocovArgs a)
{
    extern __shared__ double buf[];                // L planes of a.pitch doubles: a tile and its halo
    const int tid = threadIdx.x, nthr = blockDim.x;
    const unsigned g = blockIdx.x % (unsigned)a.ngroups;
    const unsigned sc = blockIdx.x / (unsigned)a.ngroups;
    const int c = (int)(sc % (unsigned)a.ncols), s = (int)(sc / (unsigned)a.ncols);
    const long long ra = a.start[s], rb = a.start[s + 1];
    const long long base = a.cum ? a.cum[ra] : ra;
    const long long n = (a.cum ? a.cum[rb] : rb) - base;
    const double mean = a.mean[(size_t)s * a.ncols + c];
    const int k0 = (int)g * a.group_lags + tid * L;
    double acc[L];
#pragma unroll
    for (int j = 0; j < L; j++) acc[j] = 0.0;
    for (long long t0 = 0; t0 < n; t0 += a.tile) {
        const long long left = n - t0;
        const int tl = left < a.tile ? (int)left : a.tile;
        const int len = left < a.tile + a.nlags ? (int)left : a.tile + a.nlags;
        for (long long r = bh::autocov_first_row(a.cum, ra, rb, base + t0) + tid; r < rb; r += nthr) {
            const long long at = (a.cum ? a.cum[r] : r) - base;
            if (at >= t0 + len) break;
            const long long w = a.cum ? a.cum[r + 1] - a.cum[r] : 1;
            if (w > 0) bh::autocov_expand_row(buf, L, a.pitch, t0, len, at, w, a.D[r * a.stride + c], mean);
        }
        __syncthreads();
        bh::autocov_tile<L>(buf, a.pitch, tl, left, k0, a.nlags, acc);
        __syncthreads();                           // the next tile overwrites what this one read
    }
    double *out = a.acov + ((size_t)s * a.ncols + c) * a.nlags;
    const double dn = (double)n;
#pragma unroll
    for (int j = 0; j < L; j++)
        if (k0 + j < a.nlags && k0 + j < (int)(g + 1) * a.group_lags) out[k0 + j] = n > 0 ? acc[j] / dn : 0.0;
}

}  // namespace

extern "C" int bh_autocov_sets(const double *D, long long nrows, long long stride, int ncols, const int *weights,
                               const long long *series_start, int nseries, const double *mean, int nlags, double *acov,
                               long long *length, void *stream)
{
    if (!D || nrows < 1) return bh::fail_arg_("bh_autocov_sets: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_autocov_sets: more than 2^32 rows");
    if (ncols < 1 || stride < ncols) return bh::fail_arg_("bh_autocov_sets: ncols >= 1 and stride >= ncols");
    if (nseries < 1) return bh::fail_arg_("bh_autocov_sets: one series at least");
    if (int rc = bh::check_set_start("bh_autocov_sets", series_start, nseries, nrows)) return rc;
    if (nlags < 1 || nlags > BH_AUTOCOV_MAX_LAGS) return bh::fail_arg_("bh_autocov_sets: 1 to 4096 lags");
    if (!mean || !acov || !length) return bh::fail_arg_("bh_autocov_sets: mean, acov and length");
    int tile = 0, group_lags = 0, threads = 0;
    const size_t dyn = bh::autocov_plan(nlags, &tile);
    if (dyn > (size_t)bh::kAutocovLdsBytes) return bh::fail_arg_("bh_autocov_sets: a tile and its halo do not fit the LDS");
    bh::autocov_groups(nlags, L, bh::kAutocovThreads, &group_lags, &threads);
    const int ngroups = (nlags + group_lags - 1) / group_lags;
    const size_t S = (size_t)nseries, cols = S * (size_t)ncols, cells = cols * (size_t)nlags;
    if (cols * (size_t)ngroups > 0x7fffffffull || cols * (size_t)ngroups * (size_t)threads >= (1ull << 32))
        return bh::fail_arg_("bh_autocov_sets: more than 2^31 - 1 workgroups or 2^32 threads in one launch");
    if (int rc = bh::require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    u64 neg = 0;                                   // before tmp: tmp drains the stream on every return, this one outlives it
    bh::CallBufs tmp(st);
    AutocovArgs a;
    std::memset(&a, 0, sizeof(a));
    long long *dstart = nullptr, *dcum = nullptr, *dbsum = nullptr, *dlen = nullptr;
    double *dmean = nullptr;
    u64 *dneg = nullptr;
    BH_HIP(tmp.alloc(dstart, S + 1));
    BH_HIP(tmp.alloc(dmean, cols));
    BH_HIP(tmp.alloc(a.acov, cells));
    BH_HIP(tmp.alloc(dlen, S));
    BH_HIP(tmp.alloc(dneg, 1));
    BH_HIP(hipMemcpyAsync(dstart, series_start, sizeof(long long) * (S + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dmean, mean, sizeof(double) * cols, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemsetAsync(dneg, 0, sizeof(u64), st));
    if (weights) {
        const long long nb = (nrows + kScanRows - 1) / kScanRows;
        BH_HIP(tmp.alloc(dcum, (size_t)nrows + 1));
        BH_HIP(tmp.alloc(dbsum, (size_t)nb));
        hipLaunchKernelGGL(autocov_block_sums, dim3((unsigned)nb), dim3(kScanThreads), 0, st, weights, nrows, dbsum, dneg);
        hipLaunchKernelGGL(autocov_scan_sums, dim3(1), dim3(kScanThreads), 0, st, dbsum, nb, dcum + nrows);
        hipLaunchKernelGGL(autocov_scan_rows, dim3((unsigned)nb), dim3(kScanThreads), 0, st, weights, nrows,
                           (const long long *)dbsum, dcum);
        BH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(autocov_lengths, dim3((unsigned)((nseries + 255) / 256)), dim3(256), 0, st,
                       (const long long *)dcum, (const long long *)dstart, nseries, dlen);
    BH_HIP(hipGetLastError());
    BH_HIP(hipMemcpyAsync(&neg, dneg, sizeof(u64), hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(length, dlen, sizeof(long long) * S, hipMemcpyDeviceToHost, st));
    BH_HIP(hipStreamSynchronize(st));
    if (neg) return bh::fail_arg_("bh_autocov_sets: negative weight");
    a.D = D;
    a.stride = stride;
    a.ncols = ncols;
    a.cum = dcum;
    a.start = dstart;
    a.mean = dmean;
    a.nlags = nlags;
    a.ngroups = ngroups;
    a.group_lags = group_lags;
    a.tile = tile;
    a.pitch = bh::autocov_pitch(tile, nlags, L);
    hipLaunchKernelGGL(autocov_kernel, dim3((unsigned)(cols * ngroups)), dim3((unsigned)threads), dyn, st, a);
    BH_HIP(hipGetLastError());
    BH_HIP(hipMemcpyAsync(acov, a.acov, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    BH_HIP(hipStreamSynchronize(st));
    return BH_OK;
}
