// datafits_kernel.h -- what a block of the data-fit kernels does with a range of rows: the body of df_sets_kernel
// (datafits.hip: one set per block, its own range of the rows; a bh_datafits handle is the single set of all rows),
// and the row test of the mask kernel.  The kernel hands df_block the rows [r0, r1), the block's place `bx` among the
// `G` blocks that share them, and arguments whose output pointers are the set's own; what a set's block adds up, and
// in which order, therefore depends on the set's rows alone.
//
// The part above BH_HOSTSIM's #ifndef needs no device (the launch geometry and the chunk plan of the sets):
// tests/hostsim/datafits_sets_sim.cpp compiles it with g++ (test infrastructure only).
#pragma once
#include <stdint.h>
#include "stats_core.h"

namespace bh {
namespace fit {

constexpr int kThreads = 256;
constexpr int kCols = 8;                        // columns per blockIdx.y
constexpr int kRowLanes = kThreads / kCols;     // rows a block reads at once
constexpr int kGroups = 4;                      // digit histograms per column and block (LDS 8 * 4 * 256 * 8 B = 64 KiB)
constexpr int kMaxBlocksX = 1024;               // fixed, so that the slab order depends on the row count only
constexpr int kHistLdsBytes = 64 * 1024;
constexpr int kMaxGridZ = 65535;
constexpr long long kDigitBudget = 64ll << 20;  // bytes of digit table per chunk of sets (bh_datafits_sets_set_chunk_bytes)

// blocks along the rows of a set of nrows rows (none for an empty one)
BH_HD int blocks_of(long long nrows)
{
    const long long g = (nrows + kRowLanes - 1) / kRowLanes;
    return (int)(g < kMaxBlocksX ? g : kMaxBlocksX);
}

// Sets per chunk of the select: the digit table is 256 counters per (rank, column) slot and must stay under `bytes`
// (<= 0: kDigitBudget); one set at least, and no more than the grid's z extent holds with `gz` group slices a set.
inline int sets_per_chunk(int nsets, int ncols, int nranks, int gz, long long bytes)
{
    const long long per_set = (long long)ncols * (nranks > 0 ? nranks : 1) * 256 * (long long)sizeof(uint64_t);
    long long fit = (bytes > 0 ? bytes : kDigitBudget) / per_set;
    const long long zmax = kMaxGridZ / (gz > 0 ? gz : 1);
    fit = fit > zmax ? zmax : fit;
    return (int)(fit < 1 ? 1 : fit > nsets ? nsets : fit);
}

}  // namespace fit
}  // namespace bh

#ifndef BH_HOSTSIM
#include "stats_host.h"

namespace bh {
namespace fit {

enum { MODE_SCAN = 1, MODE_FINISH = 2, MODE_RADIX = 3 };

struct FitArgs {
    const double *Y;
    long long nrows, stride;
    int ncols;
    const int *wk;                     // [nrows] effective weight (0: skip)
    double *slab;                      // [G][ncols]
    // scan
    u64 *kmin, *kmax;                  // [ncols]
    // finish
    const double *mean;                // [ncols]
    const double *edges; int nedges;   // [nsets][nedges]
    const int *eset;                   // [ncols]
    u64 *hist;                         // [ncols][nedges - 1]
    int do_hist, hist_lds;
    // radix
    int shift;                         // digit (key >> shift) & 255
    int g0;                            // the first of the kGroups groups a column's block counts (the kernel's slice)
    const int *gbase, *ngroups;        // [ncols]: first slot of the column's groups, their number
    const u64 *gpfx;                   // [slots] prefix (key >> (shift + 8)) of each group
    u64 *digits;                       // [slots][256]
};

// Σ over the 32 row lanes of each column, in lane order: thread (rl, cl) -> column cl
__device__ __forceinline__ double lanes_sum(double v, double *red, int tid)
{
    red[tid] = v;
    __syncthreads();
    double s = 0.0;
    if (tid < kCols)
        for (int l = 0; l < kRowLanes; l++) s = s + red[l * kCols + tid];
    __syncthreads();
    return s;
}

// A wave's look at row r: its weight, and whether any err flag is non-zero or any of the ncols values is NaN
// (every lane gets the answer).
__device__ __forceinline__ bool mask_row(const double *Y, long long stride, int ncols, const int *w, const int *err,
                                         int nerr, long long r, int lane, long long &wt)
{
    wt = w ? (long long)w[r] : 1;
    bool bad = false;
    const double *row = Y + r * stride;
    for (int c = lane; c < ncols; c += 64) bad |= !(row[c] == row[c]);
    if (err)
        for (int f = lane; f < nerr; f += 64) bad |= err[r * nerr + f] != 0;
    return __any(bad);
}

// Block bx of the G blocks that walk rows [r0, r1): rows r0 + bx * kRowLanes + rl, then every G * kRowLanes; the
// column tile is blockIdx.y, the slice of the select's groups a.g0.  (static: the block's LDS arrays are then
// internal to the file that includes this, and a mode that never reads one does not carry it.)
template <int MODE>
static __device__ __forceinline__ void df_block(FitArgs a, const long long r0, const long long r1, const int bx, const int G)
{
    extern __shared__ u64 lds[];
    __shared__ double red[kThreads];
    __shared__ u64 smin[kCols], smax[kCols];
    const int tid = threadIdx.x;
    const int cl = tid % kCols, rl = tid / kCols;
    const int c = blockIdx.y * kCols + cl;
    const bool valid = c < a.ncols;
    const int cc = valid ? c : a.ncols - 1;

    // radix: the groups [g0, g0 + kGroups) of this column that this block counts
    const int g0 = a.g0;
    int ng = 0, slot0 = 0;
    u64 pf[kGroups];
#pragma unroll
    for (int j = 0; j < kGroups; j++) pf[j] = 0;
    if (MODE == MODE_RADIX) {
        if (valid) {
            ng = a.ngroups[c] - g0;
            ng = ng < 0 ? 0 : (ng > kGroups ? kGroups : ng);
            slot0 = a.gbase[c] + g0;
#pragma unroll
            for (int j = 0; j < kGroups; j++) pf[j] = j < ng ? a.gpfx[slot0 + j] : 0;
        }
        // nothing to count in this slice for any column of the tile: the whole block leaves
        int any = 0;
        for (int j = 0; j < kCols; j++) {
            const int cj = blockIdx.y * kCols + j;
            any |= cj < a.ncols && a.ngroups[cj] > g0;
        }
        if (!any) return;
    }
    const bool whole = MODE == MODE_RADIX && a.shift + 8 >= 64;
    const int nb = a.nedges - 1;
    const double *ed = MODE == MODE_FINISH && a.do_hist ? a.edges + (size_t)a.eset[cc] * a.nedges : nullptr;
    const double mu = MODE == MODE_FINISH ? a.mean[cc] : 0.0;

    int nlds = 0;
    if (MODE == MODE_RADIX) nlds = kCols * kGroups * 256;
    if (MODE == MODE_FINISH && a.do_hist && a.hist_lds) nlds = kCols * nb;
    for (int i = tid; i < nlds; i += kThreads) lds[i] = 0;
    if (tid < kCols) { smin[tid] = ~0ull; smax[tid] = 0ull; }
    __syncthreads();

    double acc = 0.0;
    u64 mn = ~0ull, mx = 0ull;
    const long long step = (long long)G * kRowLanes;
    for (long long r = r0 + (long long)bx * kRowLanes + rl; r < r1; r += step) {
        const int w = a.wk[r];
        if (w == 0 || !valid) continue;
        const double y = a.Y[r * a.stride + c];
        if (MODE == MODE_SCAN) {
            acc = acc + (double)w * y;
            const u64 k = bh::post_key64(y);
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        } else if (MODE == MODE_FINISH) {
            const double e = y - mu;
            acc = acc + (double)w * (e * e);
            const int b = a.do_hist ? bh::post_bin(ed, a.nedges, y) : -1;
            if (b >= 0) {
                if (a.hist_lds) atomicAdd(&lds[cl * nb + b], (u64)w);
                else atomicAdd(&a.hist[(size_t)c * nb + b], (u64)w);
            }
        } else {
            const u64 k = bh::post_key64(y);
            const u64 hi = whole ? 0ull : (k >> (a.shift + 8));
            const int dig = (int)((k >> a.shift) & 255u);
#pragma unroll
            for (int j = 0; j < kGroups; j++)
                if (j < ng && hi == pf[j]) atomicAdd(&lds[(cl * kGroups + j) * 256 + dig], (u64)w);
        }
    }

    if (MODE != MODE_RADIX) {
        const double s = lanes_sum(acc, red, tid);
        if (tid < kCols && blockIdx.y * kCols + tid < a.ncols)
            a.slab[(size_t)bx * a.ncols + blockIdx.y * kCols + tid] = s;
    }
    if (MODE == MODE_SCAN) {
        if (mn != ~0ull) atomicMin(&smin[cl], mn);
        if (mx != 0ull) atomicMax(&smax[cl], mx);
        __syncthreads();
        if (tid < kCols && blockIdx.y * kCols + tid < a.ncols) {
            if (smin[tid] != ~0ull) atomicMin(&a.kmin[blockIdx.y * kCols + tid], smin[tid]);
            if (smax[tid] != 0ull) atomicMax(&a.kmax[blockIdx.y * kCols + tid], smax[tid]);
        }
    }
    if (MODE == MODE_FINISH && a.do_hist && a.hist_lds) {
        __syncthreads();
        for (int i = tid; i < kCols * nb; i += kThreads) {
            const int cj = blockIdx.y * kCols + i / nb;
            if (cj < a.ncols && lds[i]) atomicAdd(&a.hist[(size_t)cj * nb + i % nb], lds[i]);
        }
    }
    if (MODE == MODE_RADIX) {
        __syncthreads();
        for (int i = tid; i < kCols * kGroups * 256; i += kThreads) {
            const int cj = blockIdx.y * kCols + i / (kGroups * 256);
            const int j = (i / 256) % kGroups;
            if (cj >= a.ncols || !lds[i]) continue;
            const int n = a.ngroups[cj] - g0;
            if (j < n) atomicAdd(&a.digits[(size_t)(a.gbase[cj] + g0 + j) * 256 + (i % 256)], lds[i]);
        }
    }
}

}  // namespace fit
}  // namespace bh
#endif  // BH_HOSTSIM
