// pairs.hip -- joint histograms of column pairs for many sets of rows in one launch (bh_hist2d_sets).
//
// The two-parameter views of the sampler's scalars (bayhunter_amd/scalars.py) and the Moho trade-off of every station
// (moho.py): per set of rows (a station) and per pair of columns what np.histogram2d counts over the set's own edges.
//
//   hist2d_sets_kernel   a block belongs to one set and takes kRowsPerBlock of its rows (a long set is split over
//                        several blocks, an empty one has none: the host lists the blocks).  It copies the set's edges
//                        to LDS once, then for each group of pairs whose u64 cell tables fit beside them (pairs_core.h:
//                        pairs_plan): zero the tables, one row per lane and trip into them with LDS atomics, flush
//                        the non-zero cells to the device table with global atomics.  All pairs of a set share the
//                        block, so a station of a few hundred rows costs one block, not one per pair.
//
// Everything added is an integer: the result does not depend on the grid, the grouping or the order of arrival.
#include <cstring>
#include <string>
#include <vector>
#include "pairs_core.h"
#include "host_common.h"
#include "stats_host.h"

namespace {

using bh::u64;
constexpr int kThreads = 256;
constexpr int kRowsPerBlock = 16 * kThreads;    // a block's stretch of its set
static_assert(bh::kPairsStaticLds == sizeof(bh::PairCols) * BH_PAIRS_MAX, "the pair table is the block's static LDS");

struct AtomicAdd {
    __device__ __forceinline__ void operator()(uint64_t *cell, uint64_t wt) const { atomicAdd((u64 *)cell, (u64)wt); }
};

struct PairsArgs {
    const double *D; long long stride;
    const int *w;
    const long long *start;            // [nsets + 1]
    const int2 *blocks;                // [grid]: (set, which stretch of it)
    const bh::PairCols *pairs; int npairs, group;
    const double *edges; int nslots, ne;    // [nsets][nslots][ne]: the columns the pairs name
    u64 *hist;                         // [nsets][npairs][nb][nb]
    u64 *neg;                          // rows with a negative weight
};

__global__ __launch_bounds__(kThreads) void hist2d_sets_kernel(PairsArgs a)
{
    extern __shared__ u64 lds[];                   // edges [nslots][ne] as doubles, then `group` cell tables
    __shared__ bh::PairCols s_pair[BH_PAIRS_MAX];
    const int tid = threadIdx.x;
    const int2 blk = a.blocks[blockIdx.x];
    const int z = blk.x;
    const long long r0 = a.start[z] + (long long)blk.y * kRowsPerBlock;
    const long long rend = a.start[z + 1];
    const long long r1 = r0 + kRowsPerBlock < rend ? r0 + kRowsPerBlock : rend;
    const int ne = a.ne, nb = ne - 1, ned = a.nslots * ne;
    double *ed = (double *)lds;
    u64 *tab = lds + ned;
    const double *sed = a.edges + (size_t)z * ned;
    for (int i = tid; i < ned; i += kThreads) ed[i] = sed[i];
    if (tid < a.npairs) s_pair[tid] = a.pairs[tid];
    u64 bad = 0;
    for (int p0 = 0; p0 < a.npairs; p0 += a.group) {
        const int np = a.npairs - p0 < a.group ? a.npairs - p0 : a.group;
        const int cells = np * nb * nb;
        for (int i = tid; i < cells; i += kThreads) tab[i] = 0;
        __syncthreads();                           // the first trip: the edges and the pair table too
        for (long long r = r0 + tid; r < r1; r += kThreads) {
            const int wt = a.w ? a.w[r] : 1;
            if (wt < 0 && p0 == 0) bad++;
            if (wt <= 0) continue;
            bh::pairs_row(a.D + r * a.stride, s_pair + p0, np, ed, ne, (uint64_t)wt, (uint64_t *)tab, AtomicAdd());
        }
        __syncthreads();
        u64 *out = a.hist + ((size_t)z * a.npairs + p0) * nb * nb;
        for (int i = tid; i < cells; i += kThreads)
            if (tab[i]) atomicAdd(&out[i], tab[i]);
        __syncthreads();                           // the tables are zeroed again for the next group
    }
    if (bad) atomicAdd(a.neg, bad);
}

}  // namespace

extern "C" int bh_hist2d_sets(const double *D, long long nrows, long long stride, int ncols, const int *weights,
                              const long long *set_start, int nsets, const int *pairs, int npairs,
                              const double *edges, int nedges, long long *hist, void *stream)
{
    if (!D || nrows < 1) return bh::fail_arg_("bh_hist2d_sets: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_hist2d_sets: more than 2^32 rows (the weight total could overflow)");
    if (ncols < 1 || stride < ncols) return bh::fail_arg_("bh_hist2d_sets: ncols >= 1 and stride >= ncols");
    if (nsets < 1 || nsets > BH_PAIRS_MAX_SETS) return bh::fail_arg_("bh_hist2d_sets: 1 to 65535 sets");
    if (int rc = bh::check_set_start("bh_hist2d_sets", set_start, nsets, nrows)) return rc;
    if (npairs < 1 || npairs > BH_PAIRS_MAX || !pairs) return bh::fail_arg_("bh_hist2d_sets: 1 to 16 pairs");
    if (nedges < 2 || nedges > BH_PAIRS_MAX_EDGES) return bh::fail_arg_("bh_hist2d_sets: 2 to 65 edges");
    if (!edges || !hist) return bh::fail_arg_("bh_hist2d_sets: edges and hist");
    for (int i = 0; i < 2 * npairs; i++)
        if (pairs[i] < 0 || pairs[i] >= ncols) return bh::fail_arg_("bh_hist2d_sets: a pair's column index is out of range");
    int slot_col[2 * BH_PAIRS_MAX];
    bh::PairCols tab[BH_PAIRS_MAX];
    const int nslots = bh::pairs_slots(pairs, npairs, slot_col, tab);
    const size_t S = (size_t)nsets, ne = (size_t)nedges, nb = ne - 1;
    // the edges of the columns in use, set after set: what a block copies to its LDS
    std::vector<double> used(S * nslots * ne);
    for (size_t z = 0; z < S; z++)
        for (int s = 0; s < nslots; s++) {
            const double *e = edges + (z * (size_t)ncols + (size_t)slot_col[s]) * ne;
            if (!bh::ascending(e, nedges)) return bh::fail_arg_("bh_hist2d_sets: edges must be ascending");
            std::memcpy(&used[(z * nslots + s) * ne], e, sizeof(double) * ne);
        }
    std::vector<int2> blocks;
    for (int z = 0; z < nsets; z++) {
        const long long n = set_start[z + 1] - set_start[z];
        for (long long k = 0; k * kRowsPerBlock < n; k++) blocks.push_back(make_int2(z, (int)k));
    }
    int group = 0;
    const size_t dyn = bh::pairs_plan(nslots, nedges, npairs, &group);
    if (group < 1 || dyn + bh::kPairsStaticLds > (size_t)bh::kPairsLdsBytes)
        return bh::fail_arg_("bh_hist2d_sets: the edges and one pair's cells do not fit the LDS");
    if (int rc = bh::require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = S * (size_t)npairs * nb * nb;
    bh::CallBufs tmp(st);
    PairsArgs a;
    std::memset(&a, 0, sizeof(a));
    long long *dstart = nullptr;
    int2 *dblocks = nullptr;
    bh::PairCols *dpairs = nullptr;
    double *ded = nullptr;
    BH_HIP(tmp.alloc(dstart, S + 1));
    BH_HIP(tmp.alloc(dblocks, blocks.size()));
    BH_HIP(tmp.alloc(dpairs, (size_t)npairs));
    BH_HIP(tmp.alloc(ded, used.size()));
    BH_HIP(tmp.alloc(a.hist, cells));
    BH_HIP(tmp.alloc(a.neg, 1));
    BH_HIP(hipMemcpyAsync(dstart, set_start, sizeof(long long) * (S + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dblocks, blocks.data(), sizeof(int2) * blocks.size(), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dpairs, tab, sizeof(bh::PairCols) * npairs, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(ded, used.data(), sizeof(double) * used.size(), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemsetAsync(a.hist, 0, sizeof(u64) * cells, st));
    BH_HIP(hipMemsetAsync(a.neg, 0, sizeof(u64), st));
    a.D = D;
    a.stride = stride;
    a.w = weights;
    a.start = dstart;
    a.blocks = dblocks;
    a.pairs = dpairs;
    a.npairs = npairs;
    a.group = group;
    a.edges = ded;
    a.nslots = nslots;
    a.ne = nedges;
    hipLaunchKernelGGL(hist2d_sets_kernel, dim3((unsigned)blocks.size()), dim3(kThreads), dyn, st, a);
    BH_HIP(hipGetLastError());
    u64 neg = 0;
    BH_HIP(hipMemcpyAsync(&neg, a.neg, sizeof(u64), hipMemcpyDeviceToHost, st));
    int rc = bh::read_hist(a.hist, cells, hist, st);        // synchronises
    if (rc) return rc;
    if (neg) return bh::fail_arg_("bh_hist2d_sets: negative weight");
    return BH_OK;
}
