// posterior_kernel.h -- what a block of the posterior kernels does with a range of rows: the body of post_sets_kernel
// (posterior.hip: one set per blockIdx.z, its own range of the rows; a bh_posterior handle is the single set of all
// rows).  The kernel hands it the rows [r0, r1), the block's place `bx` among the `G` blocks that share them, and
// arguments whose output pointers are the set's own; what a set's block adds up, and in which order, therefore
// depends on the set's rows alone.
//
// The part above BH_HOSTSIM's #ifndef needs no device (the launch geometry): tests/hostsim/datafits_sets_sim.cpp
// compiles it with g++ (test infrastructure only).
#pragma once
#include <cstdint>
#include "posterior_core.h"

namespace bh {
namespace post {

constexpr int kThreads = 256;
constexpr int kTile = 8;              // depths per blockIdx.y: acc / min / max / prefixes stay in registers
constexpr int kMaxBlocksX = 1024;     // fixed, so that the slab reduction order depends on nrows only
constexpr int kHistLdsBytes = 64 * 1024;

enum { MODE_SCAN = 1, MODE_FINISH = 2 };
enum { F_ROWS = 1, F_SQ = 2, F_HIST = 4, F_RADIX = 8, F_HIST_GLOBAL = 16 };

// blocks along the rows of a set of nrows rows
BH_HD int blocks_of(long long nrows)
{
    const long long g = (nrows + kThreads - 1) / kThreads;
    return (int)(g < kMaxBlocksX ? g : kMaxBlocksX);
}

}  // namespace post
}  // namespace bh

#ifndef BH_HOSTSIM
#include "stats_host.h"

namespace bh {
namespace post {

struct PostArgs {
    const void *rows;
    long long nrows, stride;
    int width, D;
    const int *w;                      // NULL: every weight 1
    const double *misfit;              // NULL: no argmin
    const double *dep;
    int flags;
    // scan
    u64 *kmin, *kmax;                  // [D]
    double *slab;                      // [G][D]: Σ w·v (scan) or Σ w·(v-mean)² (finish)
    u64 *cnt;                          // [2]: weight total, rows with a negative weight
    u64 *nlay; int maxn;               // [maxn + 1]
    const double *ifedges; int nif;    // interface-depth edges, histogram [nif - 1]
    u64 *ifhist;
    u64 *mfkey; long long *mfrow;      // [G]
    // finish
    const double *mean;                // [D]
    const double *vedges; int nve;     // Vs edges
    const int *dbin; int ndb;          // depth bin of every grid depth (-1: outside), ndb bins
    u64 *hist;                         // [ndb][nve - 1]
    int shift;                         // radix digit (key >> shift) & 255
    const int *gbase, *ngroups;        // [D] the select's groups of each depth (one or two), stats_core.h
    const u64 *gpfx;                   // [slots] their prefixes
    u64 *digits;                       // [slots][256]
    int off_radix, off_hist, off_nlay, off_if;   // u64 offsets into the dynamic LDS
};

template <typename T> struct KeyOf;
template <> struct KeyOf<float> {
    static __device__ __forceinline__ u64 key(float v) { return bh::post_key32(v); }
    static constexpr int bits = 32;
};
template <> struct KeyOf<double> {
    static __device__ __forceinline__ u64 key(double v) { return bh::post_key64(v); }
    static constexpr int bits = 64;
};

__device__ __forceinline__ double block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

// Block bx of the G blocks that walk rows [r0, r1): row r0 + bx * kThreads + tid, then every G * kThreads.  Row
// numbers (the argmin's among them) count from the start of a.rows.
template <typename T, int MODE>
__device__ __forceinline__ void post_block(const PostArgs &a, const long long r0, const long long r1, const int bx,
                                           const int G)
{
    extern __shared__ u64 lds[];
    __shared__ double red[kThreads];
    __shared__ u64 smin[kTile], smax[kTile], swt, sneg;
    __shared__ u64 mkey[kThreads];
    __shared__ long long mrow[kThreads];
    const int tid = threadIdx.x;
    const int d0 = blockIdx.y * kTile;
    const bool rows_here = MODE == MODE_SCAN && (a.flags & F_ROWS) && blockIdx.y == 0;
    const bool do_hist = MODE == MODE_FINISH && (a.flags & F_HIST);
    const bool hist_lds = do_hist && !(a.flags & F_HIST_GLOBAL);
    const bool do_radix = MODE == MODE_FINISH && (a.flags & F_RADIX);
    const int nvb = a.nve - 1;
    const int keybits = KeyOf<T>::bits;
    const bool whole = a.shift + 8 >= keybits;       // first digit: every key matches the empty prefix

    double x[kTile], acc[kTile], mu[kTile];
    u64 mn[kTile], mx[kTile], p0[kTile], p1[kTile];
    int db[kTile];
    bool sp[kTile], valid[kTile];
    int hb0 = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < kTile; j++) {
        const int d = d0 + j;
        valid[j] = d < a.D;
        x[j] = a.dep[valid[j] ? d : a.D - 1];
        acc[j] = 0.0;
        mn[j] = ~0ull;
        mx[j] = 0ull;
        mu[j] = (MODE == MODE_FINISH && valid[j]) ? a.mean[d] : 0.0;
        db[j] = (do_hist && valid[j]) ? a.dbin[d] : -1;
        if (db[j] >= 0 && db[j] < hb0) hb0 = db[j];
        p0[j] = p1[j] = 0;
        sp[j] = false;
        if (do_radix && valid[j]) {
            p0[j] = a.gpfx[a.gbase[d]];
            sp[j] = a.ngroups[d] > 1;
            if (sp[j]) p1[j] = a.gpfx[a.gbase[d] + 1];
        }
    }
    // zero the block's LDS histograms
    int nlds = 0;
    if (do_radix) nlds = a.off_radix + kTile * 2 * 256;
    if (hist_lds) nlds = a.off_hist + kTile * nvb;
    if (rows_here) nlds = a.off_if + (a.nif > 1 ? a.nif - 1 : 0);
    for (int i = tid; i < nlds; i += kThreads) lds[i] = 0;
    if (tid < kTile) { smin[tid] = ~0ull; smax[tid] = 0ull; }
    if (tid == 0) { swt = 0; sneg = 0; }
    __syncthreads();

    u64 wsum = 0, nneg = 0;
    u64 bkey = ~0ull;
    long long brow = -1;
    const long long step = (long long)G * kThreads;
    for (long long r = r0 + (long long)bx * kThreads + tid; r < r1; r += step) {
        const long long w = a.w ? (long long)a.w[r] : 1;
        if (w <= 0) {
            if (w < 0) nneg++;
            continue;
        }
        const T *row = (const T *)a.rows + r * a.stride;
        if (rows_here && a.misfit) {
            const double m = a.misfit[r];
            const u64 k = (m != m) ? 0ull : bh::post_key64(m) + 1;    // np.argmin: the first NaN wins
            if (k < bkey) { bkey = k; brow = r; }
        }
        const int c = bh::post_row_count(row, a.width);
        if (c < 2) continue;                                           // all-NaN row: dropped
        bh::PostWalk<T> wk;
        wk.init(row, c);
        if (rows_here) {
            wsum += (u64)w;
            if (wk.n <= a.maxn) atomicAdd(&lds[a.off_nlay + wk.n], (u64)w);
            if (a.nif > 1) {
                bh::PostWalk<T> wi;
                wi.init(row, c);
                while (wi.has_interface()) {
                    const int b = bh::post_bin(a.ifedges, a.nif, wi.D);
                    if (b >= 0) atomicAdd(&lds[a.off_if + b], (u64)w);
                    wi.cross();
                }
            }
        }
        const double wd = (double)w;
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const T v = wk.at(x[j]);
            const double vd = (double)v;
            if (MODE == MODE_SCAN) {
                acc[j] = acc[j] + wd * vd;
                const u64 k = bh::post_key64(vd);
                mn[j] = k < mn[j] ? k : mn[j];
                mx[j] = k > mx[j] ? k : mx[j];
            } else {
                if (a.flags & F_SQ) {
                    const double e = vd - mu[j];
                    acc[j] = acc[j] + wd * (e * e);
                }
                if (db[j] >= 0) {
                    const int vb = bh::post_bin(a.vedges, a.nve, vd);
                    if (vb >= 0) {
                        if (hist_lds) atomicAdd(&lds[a.off_hist + (db[j] - hb0) * nvb + vb], (u64)w);
                        else atomicAdd(&a.hist[(size_t)db[j] * nvb + vb], (u64)w);
                    }
                }
                if (do_radix && valid[j]) {
                    const u64 k = KeyOf<T>::key(v);
                    const int dig = (int)((k >> a.shift) & 255u);
                    const u64 hi = whole ? 0ull : (k >> (a.shift + 8));
                    if (hi == p0[j]) atomicAdd(&lds[a.off_radix + (j * 2) * 256 + dig], (u64)w);
                    else if (sp[j] && hi == p1[j]) atomicAdd(&lds[a.off_radix + (j * 2 + 1) * 256 + dig], (u64)w);
                }
            }
        }
    }

    // ---- the block's results -------------------------------------------------------------------
    if (MODE == MODE_SCAN || (a.flags & F_SQ)) {
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const double s = block_sum(acc[j], red);
            if (tid == 0 && valid[j]) a.slab[(size_t)bx * a.D + d0 + j] = s;
        }
    }
    if (MODE == MODE_SCAN) {
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            if (mn[j] != ~0ull) atomicMin(&smin[j], mn[j]);
            if (mx[j] != 0ull) atomicMax(&smax[j], mx[j]);
        }
    }
    if (rows_here) {
        if (wsum) atomicAdd(&swt, wsum);
        if (nneg) atomicAdd(&sneg, nneg);
        mkey[tid] = bkey;
        mrow[tid] = brow;
    }
    __syncthreads();
    if (MODE == MODE_SCAN && tid < kTile && d0 + tid < a.D) {
        if (smin[tid] != ~0ull) atomicMin(&a.kmin[d0 + tid], smin[tid]);
        if (smax[tid] != 0ull) atomicMax(&a.kmax[d0 + tid], smax[tid]);
    }
    if (rows_here) {
        if (tid == 0) {
            if (swt) atomicAdd(&a.cnt[0], swt);
            if (sneg) atomicAdd(&a.cnt[1], sneg);
        }
        for (int i = tid; i <= a.maxn; i += kThreads)
            if (lds[a.off_nlay + i]) atomicAdd(&a.nlay[i], lds[a.off_nlay + i]);
        for (int i = tid; i < a.nif - 1; i += kThreads)
            if (lds[a.off_if + i]) atomicAdd(&a.ifhist[i], lds[a.off_if + i]);
        // first argmin: lexicographic (key, row) minimum, a fixed tree
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const u64 ko = mkey[tid + s];
                const long long ro = mrow[tid + s];
                if (ro >= 0 && (mrow[tid] < 0 || ko < mkey[tid] || (ko == mkey[tid] && ro < mrow[tid]))) {
                    mkey[tid] = ko;
                    mrow[tid] = ro;
                }
            }
            __syncthreads();
        }
        if (tid == 0 && a.misfit) {
            a.mfkey[bx] = mkey[0];
            a.mfrow[bx] = mrow[0];
        }
    }
    if (hist_lds && hb0 != 0x7fffffff) {
        int hb1 = hb0;
#pragma unroll
        for (int j = 0; j < kTile; j++) hb1 = db[j] > hb1 ? db[j] : hb1;
        const int n = (hb1 - hb0 + 1) * nvb;
        for (int i = tid; i < n; i += kThreads)
            if (lds[a.off_hist + i]) atomicAdd(&a.hist[(size_t)hb0 * nvb + i], lds[a.off_hist + i]);
    }
    if (do_radix) {
        for (int i = tid; i < kTile * 2 * 256; i += kThreads) {
            const int d = d0 + i / 512, t = (i / 256) % 2;
            if (d < a.D && lds[a.off_radix + i] && t < a.ngroups[d])
                atomicAdd(&a.digits[(size_t)(a.gbase[d] + t) * 256 + (i % 256)], lds[a.off_radix + i]);
        }
    }
}

// a depth tile's bins fit the kTile rows of the LDS histogram: -1 for a bin out of range, else 0 / 1
inline int tiles_fit(const int *dbin, int D, int ndbins)
{
    int fits = 1;
    for (int d0 = 0; d0 < D; d0 += kTile) {
        int lo = ndbins, hi = -1;
        for (int d = d0; d < D && d < d0 + kTile; d++) {
            if (dbin[d] < -1 || dbin[d] >= ndbins) return -1;
            if (dbin[d] >= 0) { lo = dbin[d] < lo ? dbin[d] : lo; hi = dbin[d] > hi ? dbin[d] : hi; }
        }
        if (hi >= 0 && hi - lo >= kTile) fits = 0;
    }
    return fits;
}

// the select's keys of the two middle ranks of column c -> np.median: the mean of the two middle values
inline double median_of(const RadixSelect &sel, int fp64, int c)
{
    double lo, hi;
    if (fp64) {
        lo = bh::post_unkey64(sel.key(0, c));
        hi = bh::post_unkey64(sel.key(1, c));
    } else {
        lo = (double)bh::post_unkey32((uint32_t)sel.key(0, c));
        hi = (double)bh::post_unkey32((uint32_t)sel.key(1, c));
    }
    return (lo + hi) / 2.0;
}

}  // namespace post
}  // namespace bh
#endif  // BH_HOSTSIM
