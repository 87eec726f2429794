// interfaces.hip -- discontinuity statistics of many sets of weighted rows in one pass (bh_interfaces_sets).
//
// Per set of rows (a station) and depth bin: how much weight has an interface there, a negative one, a positive one
// -- counted per interface and per model --, the joint histogram of interface depth and Vs jump, and the mean and
// spread of the jump (interfaces_core.h has the definitions and the per-row walk).
//
//   interfaces_count_kernel    a block belongs to one set and takes kIfRowsPerBlock of its rows (the host lists the
//                              blocks, an empty set has none).  One row per thread and trip; the u64 cells of a group
//                              of depth bins ([bin][6 fields + jump bins]) are privatised in LDS, updated with LDS
//                              atomics and flushed once, the non-zero cells only, with global integer atomics.  When
//                              the cells of all depth bins do not fit kIfLdsBytes the block takes the bins in groups
//                              and reads its rows once per group.  Everything added is an integer: the counts depend
//                              neither on the grid nor on the grouping nor on the order of arrival.
//   interfaces_moment_kernel   Σ w·J, and in a second launch Σ w·(J - mean)², per depth bin without floating-point
//                              atomics: each wave owns one accumulator per depth bin in LDS, and its lanes' terms are
//                              added to it by ONE lane in a fixed order (interfaces_core.h: interfaces_order), so no
//                              two updates of an accumulator race and their order is that of the set's rows.  The
//                              block's partial goes to its row of the slab, which one thread per (set, depth bin)
//                              adds in block order (stats_host.h).
//
// A set's grid is a function of its row count alone, and its blocks count from the set's first row: a set's result,
// the two sums included, is bit for bit the result of its rows alone.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "interfaces_core.h"
#include "host_common.h"
#include "stats_host.h"

namespace {

using bh::u64;
using bh::kIfThreads;
using bh::kIfRowsPerBlock;

struct AtomicAdd {
    __device__ __forceinline__ void operator()(uint64_t *cell, uint64_t wt) const { atomicAdd((u64 *)cell, (u64)wt); }
};

struct IfArgs {
    const void *rows; long long stride; int width;
    const int *w;
    const long long *start;            // [nsets + 1]
    const int2 *blocks;                // [grid]: (set, which stretch of it)
    const long long *goff;             // [nsets + 1] blocks before set z: its rows of the slab
    const double *dedges; int nde;
    const double *jedges; int nje;     // nje 0: no joint histogram
    int group;                         // depth bins per LDS table
    u64 *tab;                          // [nsets][nbd][IF_FIELDS + nbj]
    u64 *total;                        // [nsets]
    u64 *neg;                          // rows with a negative weight
    const double *mean;                // [nsets][nbd], NULL: the slab takes Σ w·J
    double *slab;                      // [blocks][nbd]
};

template <typename T>
__global__ __launch_bounds__(kIfThreads) void interfaces_count_kernel(IfArgs a)
{
    extern __shared__ u64 lds[];                   // `group` depth bins of cells
    __shared__ u64 s_total, s_neg;
    const int tid = threadIdx.x;
    const int2 blk = a.blocks[blockIdx.x];
    const int z = blk.x;
    const long long r0 = a.start[z] + (long long)blk.y * kIfRowsPerBlock;
    const long long rend = a.start[z + 1];
    const long long r1 = r0 + kIfRowsPerBlock < rend ? r0 + kIfRowsPerBlock : rend;
    const int nbd = a.nde - 1, per = bh::IF_FIELDS + (a.nje > 1 ? a.nje - 1 : 0);
    if (tid == 0) { s_total = 0; s_neg = 0; }
    u64 tot = 0, bad = 0;
    for (int d0 = 0; d0 < nbd; d0 += a.group) {
        const int nd = nbd - d0 < a.group ? nbd - d0 : a.group;
        const int cells = nd * per;
        for (int i = tid; i < cells; i += kIfThreads) lds[i] = 0;
        __syncthreads();                           // the first trip: the two counters too
        for (long long r = r0 + tid; r < r1; r += kIfThreads) {
            const int wt = a.w ? a.w[r] : 1;
            if (d0 == 0) {
                if (wt < 0) bad++;
                else tot += (u64)wt;
            }
            if (wt <= 0) continue;
            bh::interfaces_row((const T *)a.rows + r * a.stride, a.width, (uint64_t)wt, a.dedges, a.nde, a.jedges,
                               a.nje, d0, d0 + nd, (uint64_t *)lds, AtomicAdd());
        }
        __syncthreads();
        u64 *out = a.tab + ((size_t)z * nbd + d0) * per;
        for (int i = tid; i < cells; i += kIfThreads)
            if (lds[i]) atomicAdd(&out[i], lds[i]);
        __syncthreads();                           // the cells are zeroed again for the next group
    }
    if (tot) atomicAdd(&s_total, tot);
    if (bad) atomicAdd(&s_neg, bad);
    __syncthreads();
    if (tid == 0) {
        if (s_total) atomicAdd(&a.total[z], s_total);
        if (s_neg) atomicAdd(a.neg, s_neg);
    }
}

template <typename T>
__global__ __launch_bounds__(kIfThreads) void interfaces_moment_kernel(IfArgs a)
{
    extern __shared__ double acc[];                // [kIfWaves][nbd]
    const int tid = threadIdx.x, lane = tid & (bh::kIfWave - 1), wave = tid / bh::kIfWave;
    const int2 blk = a.blocks[blockIdx.x];
    const int z = blk.x;
    const long long r0 = a.start[z] + (long long)blk.y * kIfRowsPerBlock;
    const long long rend = a.start[z + 1];
    const long long r1 = r0 + kIfRowsPerBlock < rend ? r0 + kIfRowsPerBlock : rend;
    const int nbd = a.nde - 1;
    const double *mean = a.mean ? a.mean + (size_t)z * nbd : nullptr;
    for (int i = tid; i < bh::kIfWaves * nbd; i += kIfThreads) acc[i] = 0.0;
    __syncthreads();
    double *mine = acc + wave * nbd;
    for (int t = 0; t < bh::kIfTrips; t++) {       // every wave makes every trip: its lanes vote below
        const long long r = r0 + (long long)t * kIfThreads + tid;
        const int wt = r < r1 ? (a.w ? a.w[r] : 1) : 0;
        const T *row = (const T *)a.rows + (r < r1 ? r : r0) * a.stride;
        bh::PostWalk<T> wk;
        wk.init(row, wt > 0 ? bh::post_row_count(row, a.width) : 0);
        bool open = wk.has_interface();
        while (__any(open)) {                      // interface k of every row of the wave
            int d = -1;
            double v = 0.0;
            if (open) {
                d = bh::post_bin(a.dedges, a.nde, wk.D);
                if (d >= 0) v = bh::interfaces_term((double)wt, bh::interfaces_jump(wk), mean, d);
                wk.cross();
                open = wk.has_interface();
            }
            u64 todo = __ballot(d >= 0);
            while (todo) {                         // lanes ascending; lane 0 alone touches the wave's accumulators
                const int src = __ffsll((unsigned long long)todo) - 1;
                const int dd = __shfl(d, src, bh::kIfWave);
                const double vv = __shfl(v, src, bh::kIfWave);
                if (lane == 0) mine[dd] = mine[dd] + vv;
                todo &= todo - 1;
            }
        }
    }
    __syncthreads();
    double *out = a.slab + (size_t)(a.goff[z] + blk.y) * nbd;
    for (int i = tid; i < nbd; i += kIfThreads)
        out[i] = ((acc[i] + acc[nbd + i]) + acc[2 * nbd + i]) + acc[3 * nbd + i];
}
static_assert(bh::kIfWaves == 4, "the block's partial is written out for four waves");

bool finite_ascending(const double *v, int n)
{
    return bh::ascending(v, n) && std::isfinite(v[0]) && std::isfinite(v[n - 1]);
}

template <typename T>
int launch_moments(const IfArgs &a, size_t nblocks, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL(interfaces_moment_kernel<T>, dim3((unsigned)nblocks), dim3(kIfThreads), lds, st, a);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

}  // namespace

extern "C" int bh_interfaces_sets(const void *rows, int fp64, long long nrows, long long stride, int width,
                                  const int *weights, const long long *set_start, int nsets, const double *dedges,
                                  int ndedges, const double *jedges, int njedges, long long *total, long long *count,
                                  long long *models, long long *neg, long long *pos, long long *models_neg,
                                  long long *models_pos, long long *hist, double *jsum, double *jsq, void *stream)
{
    const char *who = "bh_interfaces_sets";
    if (!rows || nrows < 1) return bh::fail_who(who, "no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_who(who, "more than 2^32 rows (the weight total could overflow)");
    if (width < 2 || width > 2 * BH_MAX_LAYERS + 2 || stride < width) return bh::fail_who(who, "width / stride");
    if (nsets < 1 || nsets > BH_PAIRS_MAX_SETS) return bh::fail_who(who, "1 to 65535 sets");
    if (int rc = bh::check_set_start(who, set_start, nsets, nrows)) return rc;
    if (!dedges || ndedges < 2 || ndedges > BH_INTERFACES_MAX_DEPTH_BINS + 1)
        return bh::fail_who(who, "depth edges: 2 to 1025");
    if (!finite_ascending(dedges, ndedges)) return bh::fail_who(who, "depth edges must be finite and ascending");
    if (!jedges) njedges = 0;
    if (jedges && (njedges < 2 || njedges > BH_INTERFACES_MAX_JUMP_BINS + 1))
        return bh::fail_who(who, "jump edges: 2 to 257, or none");
    if (jedges && !finite_ascending(jedges, njedges)) return bh::fail_who(who, "jump edges must be finite and ascending");
    if (hist && !jedges) return bh::fail_who(who, "hist needs jump edges");
    if (int rc = bh::require_device()) return rc;

    hipStream_t st = (hipStream_t)stream;
    const size_t S = (size_t)nsets, nbd = (size_t)ndedges - 1, nbj = jedges ? (size_t)njedges - 1 : 0;
    const size_t per = bh::IF_FIELDS + nbj, cells = S * nbd * per;
    std::vector<int2> blocks;
    std::vector<long long> goff(S + 1, 0);
    for (int z = 0; z < nsets; z++) {
        const int g = bh::interfaces_blocks_of(set_start[z + 1] - set_start[z]);
        goff[z + 1] = goff[z] + g;
        for (int k = 0; k < g; k++) blocks.push_back(make_int2(z, k));
    }
    bh::CallBufs tmp(st);
    IfArgs a;
    std::memset(&a, 0, sizeof(a));
    long long *dstart = nullptr, *dgoff = nullptr;
    int2 *dblocks = nullptr;
    double *ded = nullptr, *dmean = nullptr, *dred = nullptr;
    BH_HIP(tmp.alloc(dstart, S + 1));
    BH_HIP(tmp.alloc(dgoff, S + 1));
    BH_HIP(tmp.alloc(dblocks, blocks.size()));
    BH_HIP(tmp.alloc(ded, (size_t)ndedges + njedges));
    BH_HIP(tmp.alloc(a.tab, cells));
    BH_HIP(tmp.alloc(a.total, S));
    BH_HIP(tmp.alloc(a.neg, 1));
    BH_HIP(hipMemcpyAsync(dstart, set_start, sizeof(long long) * (S + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dgoff, goff.data(), sizeof(long long) * (S + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dblocks, blocks.data(), sizeof(int2) * blocks.size(), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(ded, dedges, sizeof(double) * ndedges, hipMemcpyHostToDevice, st));
    if (jedges) BH_HIP(hipMemcpyAsync(ded + ndedges, jedges, sizeof(double) * njedges, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemsetAsync(a.tab, 0, sizeof(u64) * cells, st));
    BH_HIP(hipMemsetAsync(a.total, 0, sizeof(u64) * S, st));
    BH_HIP(hipMemsetAsync(a.neg, 0, sizeof(u64), st));
    a.rows = rows;
    a.stride = stride;
    a.width = width;
    a.w = weights;
    a.start = dstart;
    a.blocks = dblocks;
    a.goff = dgoff;
    a.dedges = ded;
    a.nde = ndedges;
    a.jedges = jedges ? ded + ndedges : nullptr;
    a.nje = njedges;
    a.group = bh::interfaces_group((int)nbd, (int)nbj);
    const size_t lds = sizeof(u64) * (size_t)a.group * per;
    if (fp64)
        hipLaunchKernelGGL(interfaces_count_kernel<double>, dim3((unsigned)blocks.size()), dim3(kIfThreads), lds, st, a);
    else
        hipLaunchKernelGGL(interfaces_count_kernel<float>, dim3((unsigned)blocks.size()), dim3(kIfThreads), lds, st, a);
    BH_HIP(hipGetLastError());
    std::vector<u64> tab(cells), tot(S);
    u64 bad = 0;
    BH_HIP(hipMemcpyAsync(tab.data(), a.tab, sizeof(u64) * cells, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(tot.data(), a.total, sizeof(u64) * S, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(&bad, a.neg, sizeof(u64), hipMemcpyDeviceToHost, st));
    BH_HIP(hipStreamSynchronize(st));
    if (bad) return bh::fail_who(who, "negative weight");

    long long *fields[bh::IF_FIELDS] = {count, models, neg, pos, models_neg, models_pos};
    for (size_t z = 0; z < S; z++) {
        if (total) total[z] = (long long)tot[z];
        for (size_t d = 0; d < nbd; d++) {
            const u64 *cell = &tab[(z * nbd + d) * per];
            for (int f = 0; f < bh::IF_FIELDS; f++)
                if (fields[f]) fields[f][z * nbd + d] = (long long)cell[f];
            if (hist)
                for (size_t j = 0; j < nbj; j++) hist[(z * nbd + d) * nbj + j] = (long long)cell[bh::IF_FIELDS + j];
        }
    }
    if (!jsum && !jsq) return BH_OK;

    // the two sums: one launch each, the slab added per set in block order
    const size_t mlds = sizeof(double) * bh::kIfWaves * nbd;
    const size_t ncol = S * nbd;
    std::vector<double> sum(ncol), mu(ncol), sq;
    BH_HIP(tmp.alloc(a.slab, (size_t)goff[S] * nbd));
    BH_HIP(tmp.alloc(dred, ncol));
    for (int pass = 0; pass < (jsq ? 2 : 1); pass++) {
        if (pass == 1) {
            for (size_t i = 0; i < ncol; i++) {
                const u64 c = tab[i * per + bh::IF_COUNT];
                mu[i] = c ? sum[i] / (double)c : std::nan("");
            }
            BH_HIP(tmp.alloc(dmean, ncol));
            BH_HIP(hipMemcpyAsync(dmean, mu.data(), sizeof(double) * ncol, hipMemcpyHostToDevice, st));
            a.mean = dmean;
        }
        if (int rc = fp64 ? launch_moments<double>(a, blocks.size(), mlds, st)
                          : launch_moments<float>(a, blocks.size(), mlds, st))
            return rc;
        hipLaunchKernelGGL(bh::stats_sets_reduce_kernel<double>, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, st,
                           (const double *)a.slab, (const long long *)dgoff, nsets, (int)nbd, dred);
        BH_HIP(hipGetLastError());
        std::vector<double> &out = pass ? sq : sum;
        out.resize(ncol);
        BH_HIP(hipMemcpyAsync(out.data(), dred, sizeof(double) * ncol, hipMemcpyDeviceToHost, st));
        BH_HIP(hipStreamSynchronize(st));
    }
    for (size_t z = 0; z < S; z++)
        for (size_t d = 0; d < nbd; d++) {
            const size_t i = z * nbd + d;
            if (jsum) jsum[i] = tot[z] ? sum[i] : std::nan("");
            if (jsq) jsq[i] = tot[z] ? sq[i] : std::nan("");
        }
    return BH_OK;
}
