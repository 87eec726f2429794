// moho.hip -- Moho depth and crustal velocity of a block of weighted rows (bh_moho_*).
//
// The reference derives them in PlotFromStorage.plot_moho_crustvel_tradeoff (src/Plotting.py:753-902): a Python
// loop over the posterior models (:766-798), then medians, a standard deviation, four histograms and three joint
// histograms against the Moho depth (:813-865).  Here:
//
//   moho_rows_kernel     one row per lane -> D[row][4] = (moho, vs_crust, vs_last, vs_jump) in fp64, NaN without a
//                        Moho (moho_core.h: bit for bit what numpy computes from the row in the row's dtype)
//   moho_hist2d_kernel   the three joint histograms (x: vs_last, vs_crust, vs_jump; y: moho) over D with integer
//                        weights in one launch: u64 counts privatised in LDS (3 * nb * nb * 8 B, 60 000 B at 50
//                        bins), global atomics when they do not fit
//   moho_sets_kernel     one workgroup per contiguous set of rows (a station): weight totals with and without a
//                        Moho, min / max / mean / population std and the two middle order statistics of the four
//                        columns, and the histogram of the Moho depth over edges all sets share.  All passes run
//                        inside the kernel (sums and keys; squares and histogram; eight 8-bit radix passes over
//                        256-bin u64 digit tables in LDS), nothing returns to the host in between.
//
// The statistics of a single set are the weighted column reduction of datafits.hip over D (Y = D, ncols = 4): a
// row of NaN is one of its excluded rows.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "moho_core.h"
#include "host_common.h"
#include "stats_host.h"

namespace {

using bh::u64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kHist2dLdsBytes = 64 * 1024;       // moho_hist2d_kernel has no static LDS
constexpr int kHist2dBlocks = 256;               // each block zeroes and flushes its private tables
constexpr int kSetHistLdsBins = 2048;            // moho_sets_kernel: 16 KiB of histogram beside its 16 KiB of digits
constexpr int kStats = 6;                        // per (set, column): min, max, mean, std, lower / upper middle

template <typename T>
__global__ __launch_bounds__(kThreads) void moho_rows_kernel(const T *rows, long long nrows, long long stride,
                                                            int width, double zlo, double zhi, double mohovs,
                                                            double *out)
{
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= nrows) return;
    double d[4];
    bh::moho_row(rows + r * stride, width, zlo, zhi, mohovs, d);
    double *o = out + 4 * r;
    o[0] = d[0];
    o[1] = d[1];
    o[2] = d[2];
    o[3] = d[3];
}

// D[nrows][4]; xedges[3][ne] for the columns 2, 1, 3 (vs_last, vs_crust, vs_jump), yedges[ne] for column 0;
// hist[3][nb][nb] with the x bin first; neg: rows with a negative weight
__global__ __launch_bounds__(kThreads) void moho_hist2d_kernel(const double *D, long long nrows, const int *w,
                                                              const double *xedges, const double *yedges, int ne,
                                                              u64 *hist, int use_lds, u64 *neg)
{
    extern __shared__ u64 lds[];
    const int nb = ne - 1;
    const int cells = 3 * nb * nb;
    if (use_lds) {
        for (int i = threadIdx.x; i < cells; i += kThreads) lds[i] = 0;
        __syncthreads();
    }
    u64 *tab = use_lds ? lds : hist;
    u64 bad = 0;
    const long long step = (long long)gridDim.x * kThreads;
    for (long long r = (long long)blockIdx.x * kThreads + threadIdx.x; r < nrows; r += step) {
        const int wt = w ? w[r] : 1;
        if (wt < 0) bad++;
        if (wt <= 0) continue;
        const double *d = D + 4 * r;
        const double y = d[0], x0 = d[2], x1 = d[1], x2 = d[3];
        if (!(y == y) || !(x0 == x0) || !(x1 == x1) || !(x2 == x2)) continue;
        const int by = bh::post_bin(yedges, ne, y);
        if (by < 0) continue;
        const int b0 = bh::post_bin(xedges, ne, x0);
        const int b1 = bh::post_bin(xedges + ne, ne, x1);
        const int b2 = bh::post_bin(xedges + 2 * ne, ne, x2);
        if (b0 >= 0) atomicAdd(&tab[(0 * nb + b0) * nb + by], (u64)wt);
        if (b1 >= 0) atomicAdd(&tab[(1 * nb + b1) * nb + by], (u64)wt);
        if (b2 >= 0) atomicAdd(&tab[(2 * nb + b2) * nb + by], (u64)wt);
    }
    if (bad) atomicAdd(neg, bad);
    if (use_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += kThreads)
            if (lds[i]) atomicAdd(&hist[i], lds[i]);
    }
}

// Σ over the block in a fixed tree; every thread gets the sum
__device__ __forceinline__ double block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

struct SetsArgs {
    const double *D;
    const int *w;
    const long long *start;            // [nsets + 1]
    const double *edges; int ne;       // shared edges of the Moho histogram (ne 0: none)
    u64 *cnt;                          // [nsets][2] weight with / without a Moho
    double *stats;                     // [nsets][4][kStats]
    u64 *hist;                         // [nsets][ne - 1]
    u64 *flags;                        // [2] rows with a negative weight; sets with a weight total above 2^53
    int hist_lds;
};

// one workgroup per set; a thread takes the rows r0 + tid, r0 + tid + 256, ... of its set, so nothing it adds
// depends on where the set lies or on how many sets there are
__global__ __launch_bounds__(kThreads) void moho_sets_kernel(SetsArgs a)
{
    extern __shared__ u64 shist[];                 // [ne - 1] when hist_lds
    __shared__ u64 digits[4 * 2 * 256];            // [column][rank][digit]
    __shared__ double red[kThreads];
    __shared__ u64 s_cnt[3], s_min[4], s_max[4], s_pfx[8], s_left[8];
    const int tid = threadIdx.x, z = blockIdx.x;
    const long long r0 = a.start[z], r1 = a.start[z + 1];
    const int nb = a.ne > 1 ? a.ne - 1 : 0;
    const double nan = __builtin_nan("");

    if (tid < 3) s_cnt[tid] = 0;
    if (tid < 4) { s_min[tid] = ~0ull; s_max[tid] = 0ull; }
    if (a.hist_lds)
        for (int i = tid; i < nb; i += kThreads) shist[i] = 0;
    else
        for (int i = tid; i < nb; i += kThreads) a.hist[(size_t)z * nb + i] = 0;
    __syncthreads();

    // pass 1: weight totals, Σ w v, min / max keys
    u64 in = 0, ex = 0, neg = 0;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    u64 mn[4] = {~0ull, ~0ull, ~0ull, ~0ull}, mx[4] = {0ull, 0ull, 0ull, 0ull};
    for (long long r = r0 + tid; r < r1; r += kThreads) {
        const int wt = a.w ? a.w[r] : 1;
        if (wt < 0) { neg++; continue; }
        const double *d = a.D + 4 * r;
        const double v[4] = {d[0], d[1], d[2], d[3]};
        if (!(v[0] == v[0]) || !(v[1] == v[1]) || !(v[2] == v[2]) || !(v[3] == v[3])) { ex += (u64)wt; continue; }
        if (wt == 0) continue;
        in += (u64)wt;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            sum[c] = sum[c] + (double)wt * v[c];
            const u64 k = bh::post_key64(v[c]);
            mn[c] = k < mn[c] ? k : mn[c];
            mx[c] = k > mx[c] ? k : mx[c];
        }
    }
    if (in) atomicAdd(&s_cnt[0], in);
    if (ex) atomicAdd(&s_cnt[1], ex);
    if (neg) atomicAdd(&s_cnt[2], neg);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (mn[c] != ~0ull) atomicMin(&s_min[c], mn[c]);
        if (mx[c] != 0ull) atomicMax(&s_max[c], mx[c]);
    }
    double mean[4];
#pragma unroll
    for (int c = 0; c < 4; c++) mean[c] = block_sum(sum[c], red);      // synchronises: s_cnt is complete after it
    const u64 W = s_cnt[0];
    if (tid == 0) {
        a.cnt[2 * (size_t)z] = W;
        a.cnt[2 * (size_t)z + 1] = s_cnt[1];
        if (s_cnt[2]) atomicAdd(&a.flags[0], s_cnt[2]);
        if (W > (1ull << 53)) atomicAdd(&a.flags[1], 1ull);
    }
    double *st = a.stats + (size_t)z * 4 * kStats;
    if (W == 0 || W > (1ull << 53)) {              // a hole of the map: the same for the whole block
        if (tid < 4 * kStats) st[tid] = nan;
        if (a.hist_lds)                            // the global form zeroed its histogram above
            for (int i = tid; i < nb; i += kThreads) a.hist[(size_t)z * nb + i] = 0;
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) mean[c] = mean[c] / (double)W;

    // pass 2: Σ w (v - mean)², the histogram of the Moho depth
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long r = r0 + tid; r < r1; r += kThreads) {
        const int wt = a.w ? a.w[r] : 1;
        if (wt <= 0) continue;
        const double *d = a.D + 4 * r;
        const double v[4] = {d[0], d[1], d[2], d[3]};
        if (!(v[0] == v[0]) || !(v[1] == v[1]) || !(v[2] == v[2]) || !(v[3] == v[3])) continue;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const double e = v[c] - mean[c];
            sq[c] = sq[c] + (double)wt * (e * e);
        }
        if (nb) {
            const int b = bh::post_bin(a.edges, a.ne, v[0]);
            if (b >= 0) {
                if (a.hist_lds) atomicAdd(&shist[b], (u64)wt);
                else atomicAdd(&a.hist[(size_t)z * nb + b], (u64)wt);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) sq[c] = block_sum(sq[c], red);
    if (tid < 4) {
        const double m = tid == 0 ? mean[0] : tid == 1 ? mean[1] : tid == 2 ? mean[2] : mean[3];
        const double q = tid == 0 ? sq[0] : tid == 1 ? sq[1] : tid == 2 ? sq[2] : sq[3];
        st[tid * kStats + 0] = bh::post_unkey64(s_min[tid]);
        st[tid * kStats + 1] = bh::post_unkey64(s_max[tid]);
        st[tid * kStats + 2] = m;
        st[tid * kStats + 3] = sqrt(q / (double)W);
    }
    if (a.hist_lds)                                // block_sum synchronised after the last shist update
        for (int i = tid; i < nb; i += kThreads) a.hist[(size_t)z * nb + i] = shist[i];

    // the two middle order statistics (0-based ranks (W - 1) / 2 and W / 2) of every column: an 8-bit radix select
    // from the most significant digit; table (c, j) counts the keys that share the prefix found so far for rank j
    if (tid < 8) {
        s_pfx[tid] = 0;
        s_left[tid] = (tid & 1) ? W / 2 : (W - 1) / 2;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < 4 * 2 * 256; i += kThreads) digits[i] = 0;
        __syncthreads();
        u64 pf[8];
#pragma unroll
        for (int i = 0; i < 8; i++) pf[i] = s_pfx[i];
        for (long long r = r0 + tid; r < r1; r += kThreads) {
            const int wt = a.w ? a.w[r] : 1;
            if (wt <= 0) continue;
            const double *d = a.D + 4 * r;
            const double v[4] = {d[0], d[1], d[2], d[3]};
            if (!(v[0] == v[0]) || !(v[1] == v[1]) || !(v[2] == v[2]) || !(v[3] == v[3])) continue;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const u64 k = bh::post_key64(v[c]);
                const u64 hi = shift == 56 ? 0ull : (k >> (shift + 8));
                const int dig = (int)((k >> shift) & 255u);
#pragma unroll
                for (int j = 0; j < 2; j++)
                    if (hi == pf[2 * c + j]) atomicAdd(&digits[(2 * c + j) * 256 + dig], (u64)wt);
            }
        }
        __syncthreads();
        // wave v walks the tables v and v + 4: lane l owns the digits 4 l .. 4 l + 3; the lane whose span holds
        // the rank finds the digit
        const int lane = tid & 63, wave = tid >> 6;
        for (int t = wave; t < 8; t += kWaves) {
            const u64 *h = digits + t * 256 + 4 * lane;
            const u64 h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
            const u64 mine = h0 + h1 + h2 + h3;
            u64 incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const u64 up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            const u64 excl = incl - mine, left = s_left[t];
            if (left >= excl && left < incl) {     // exactly one lane: the table's total is above the rank
                u64 cum = excl;
                int b = 0;
                if (cum + h0 <= left) { cum += h0; b = 1;
                    if (cum + h1 <= left) { cum += h1; b = 2;
                        if (cum + h2 <= left) { cum += h2; b = 3; } } }
                s_pfx[t] = (s_pfx[t] << 8) | (u64)(4 * lane + b);
                s_left[t] = left - cum;
            }
        }
        __syncthreads();
    }
    if (tid < 8) st[(tid >> 1) * kStats + 4 + (tid & 1)] = bh::post_unkey64(s_pfx[tid]);
}

}  // namespace

extern "C" {

int bh_moho_rows(const void *rows, int fp64, long long nrows, long long stride, int width, double zlo, double zhi,
                 double mohovs, double *out, void *stream)
{
    if (!rows || !out) return bh::fail_arg_("bh_moho_rows: rows or out is NULL");
    if (nrows < 1) return bh::fail_arg_("bh_moho_rows: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_moho_rows: more than 2^32 rows");
    if (width < 2 || width > 2 * BH_MAX_LAYERS + 2 || stride < width) return bh::fail_arg_("bh_moho_rows: width / stride");
    if (!(zlo < zhi)) return bh::fail_arg_("bh_moho_rows: the depth window needs zlo < zhi");
    if (!(mohovs == mohovs)) return bh::fail_arg_("bh_moho_rows: mohovs is NaN");
    if (int rc = bh::require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((nrows + kThreads - 1) / kThreads));
    if (fp64)
        hipLaunchKernelGGL(moho_rows_kernel<double>, grid, dim3(kThreads), 0, st, (const double *)rows, nrows, stride,
                           width, zlo, zhi, mohovs, out);
    else
        hipLaunchKernelGGL(moho_rows_kernel<float>, grid, dim3(kThreads), 0, st, (const float *)rows, nrows, stride,
                           width, zlo, zhi, mohovs, out);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

int bh_moho_hist2d(const double *D, long long nrows, const int *weights, const double *xedges, const double *yedges,
                   int nedges, long long *hist, void *stream)
{
    if (!D || nrows < 1) return bh::fail_arg_("bh_moho_hist2d: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_moho_hist2d: more than 2^32 rows (the weight total could overflow)");
    if (!xedges || !yedges || !hist) return bh::fail_arg_("bh_moho_hist2d: xedges, yedges and hist");
    if (nedges < 2 || nedges > 4097) return bh::fail_arg_("bh_moho_hist2d: 2 to 4097 edges");
    for (int s = 0; s < 3; s++)
        if (!bh::ascending(xedges + (size_t)s * nedges, nedges)) return bh::fail_arg_("bh_moho_hist2d: edges must be ascending");
    if (!bh::ascending(yedges, nedges)) return bh::fail_arg_("bh_moho_hist2d: edges must be ascending");
    if (int rc = bh::require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nb = nedges - 1;
    const size_t cells = 3 * (size_t)nb * nb;
    bh::CallBufs tmp(st);
    double *ded = nullptr;
    u64 *dh = nullptr, *dneg = nullptr;
    BH_HIP(tmp.alloc(ded, 4 * (size_t)nedges));
    BH_HIP(tmp.alloc(dh, cells));
    BH_HIP(tmp.alloc(dneg, 1));
    BH_HIP(hipMemcpyAsync(ded, xedges, sizeof(double) * 3 * nedges, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(ded + 3 * (size_t)nedges, yedges, sizeof(double) * nedges, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemsetAsync(dh, 0, sizeof(u64) * cells, st));
    BH_HIP(hipMemsetAsync(dneg, 0, sizeof(u64), st));
    const int use_lds = cells * sizeof(u64) <= (size_t)kHist2dLdsBytes;
    const long long blocks = (nrows + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(moho_hist2d_kernel, dim3((unsigned)(blocks < kHist2dBlocks ? blocks : kHist2dBlocks)),
                       dim3(kThreads), use_lds ? cells * sizeof(u64) : 0, st, D, nrows, weights, (const double *)ded,
                       (const double *)(ded + 3 * (size_t)nedges), nedges, dh, use_lds, dneg);
    BH_HIP(hipGetLastError());
    u64 neg = 0;
    BH_HIP(hipMemcpyAsync(&neg, dneg, sizeof(u64), hipMemcpyDeviceToHost, st));
    int rc = bh::read_hist(dh, cells, hist, st);           // synchronises
    if (rc) return rc;
    if (neg) return bh::fail_arg_("bh_moho_hist2d: negative weight");
    return BH_OK;
}

int bh_moho_sets(const double *D, long long nrows, const int *weights, const long long *set_start, int nsets,
                 const double *edges, int nedges, long long *with_moho, long long *without, double *vmin,
                 double *vmax, double *mean, double *stdev, double *medlo, double *medhi, long long *hist,
                 void *stream)
{
    if (!D || nrows < 1) return bh::fail_arg_("bh_moho_sets: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_moho_sets: more than 2^32 rows (the weight total could overflow)");
    if (nsets < 1 || nsets > (1 << 24)) return bh::fail_arg_("bh_moho_sets: 1 to 2^24 sets");
    if (int rc = bh::check_set_start("bh_moho_sets", set_start, nsets, nrows)) return rc;
    const bool want_hist = edges != nullptr;
    if (want_hist && (nedges < 2 || !hist || !bh::ascending(edges, nedges)))
        return bh::fail_arg_("bh_moho_sets: edges must be ascending, two at least, with hist");
    if (int rc = bh::require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nb = want_hist ? nedges - 1 : 0;
    const size_t S = (size_t)nsets;
    bh::CallBufs tmp(st);
    SetsArgs a;
    std::memset(&a, 0, sizeof(a));
    long long *dstart = nullptr;
    double *ded = nullptr;
    BH_HIP(tmp.alloc(dstart, S + 1));
    BH_HIP(tmp.alloc(a.cnt, 2 * S));
    BH_HIP(tmp.alloc(a.stats, S * 4 * kStats));
    BH_HIP(tmp.alloc(a.flags, 2));
    BH_HIP(hipMemcpyAsync(dstart, set_start, sizeof(long long) * (S + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemsetAsync(a.flags, 0, sizeof(u64) * 2, st));
    if (want_hist) {
        BH_HIP(tmp.alloc(ded, nedges));
        BH_HIP(tmp.alloc(a.hist, S * nb));
        BH_HIP(hipMemcpyAsync(ded, edges, sizeof(double) * nedges, hipMemcpyHostToDevice, st));
    }
    a.D = D;
    a.w = weights;
    a.start = dstart;
    a.edges = ded;
    a.ne = want_hist ? nedges : 0;
    a.hist_lds = nb <= kSetHistLdsBins;
    hipLaunchKernelGGL(moho_sets_kernel, dim3((unsigned)nsets), dim3(kThreads), a.hist_lds ? sizeof(u64) * nb : 0, st, a);
    BH_HIP(hipGetLastError());
    std::vector<u64> cnt(2 * S);
    std::vector<double> stt(S * 4 * kStats);
    u64 flags[2] = {0, 0};
    BH_HIP(hipMemcpyAsync(cnt.data(), a.cnt, sizeof(u64) * 2 * S, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(stt.data(), a.stats, sizeof(double) * S * 4 * kStats, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(flags, a.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    if (want_hist) {
        int rc = bh::read_hist(a.hist, S * nb, hist, st);   // synchronises
        if (rc) return rc;
    } else {
        BH_HIP(hipStreamSynchronize(st));
    }
    if (flags[0]) return bh::fail_arg_("bh_moho_sets: negative weight");
    if (flags[1]) return bh::fail_arg_("bh_moho_sets: weight total above 2^53");
    double *outs[kStats] = {vmin, vmax, mean, stdev, medlo, medhi};
    for (size_t z = 0; z < S; z++) {
        if (with_moho) with_moho[z] = (long long)cnt[2 * z];
        if (without) without[z] = (long long)cnt[2 * z + 1];
        for (int c = 0; c < 4; c++)
            for (int k = 0; k < kStats; k++)
                if (outs[k]) outs[k][4 * z + c] = stt[(z * 4 + c) * kStats + k];
    }
    return BH_OK;
}

}  // extern "C"
