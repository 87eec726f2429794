// stats_core.h -- what the weighted column reductions (posterior.hip, datafits.hip) share and that needs no
// device: the order-preserving keys, the bin search, and the host side of the radix select.
//
// No HIP calls.  Compiled with g++ under BH_HOSTSIM by tests/hostsim/posterior_sim.cpp (test infrastructure
// only), which is how the CPU tier drives the select.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "bh_common.h"

namespace bh {

// order-preserving unsigned keys: a < b  <=>  key(a) < key(b) for every non-NaN value (-0 < +0)
BH_HD uint64_t post_key64(double v)
{
    union { double d; uint64_t u; } c;
    c.d = v;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
BH_HD double post_unkey64(uint64_t k)
{
    union { double d; uint64_t u; } c;
    c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.d;
}
BH_HD uint32_t post_key32(float v)
{
    union { float f; uint32_t u; } c;
    c.f = v;
    return (c.u >> 31) ? ~c.u : (c.u | 0x80000000u);
}
BH_HD float post_unkey32(uint32_t k)
{
    union { float f; uint32_t u; } c;
    c.u = (k >> 31) ? (k & 0x7fffffffu) : ~k;
    return c.f;
}

// Bin of v among ascending edges[0..ne): i with edges[i] <= v < edges[i+1], the last bin closed on the
// right, -1 outside (NaN included) -- numpy's searchsorted(side='right') - 1 with its last-edge fix.
BH_HD int post_bin(const double *edges, int ne, double v)
{
    if (!(v >= edges[0]) || !(v <= edges[ne - 1])) return -1;
    if (v == edges[ne - 1]) return ne - 2;
    int lo = 0, hi = ne;              // first index with edges[i] > v lies in (lo, hi]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The slab of the segmented reductions (stats_host.h: SetStats): set z owns blocks_of(its rows) slab rows from goff[z],
// an empty set none, and goff[nsets] rows are the slab.  -> the blocks of the largest set, 1 at least (a grid extent)
inline int set_slab_offsets(const long long *start, int nsets, int (*blocks_of)(long long), long long *goff)
{
    int gmax = 1;
    goff[0] = 0;
    for (int z = 0; z < nsets; z++) {
        const int g = blocks_of(start[z + 1] - start[z]);
        goff[z + 1] = goff[z] + g;
        gmax = g > gmax ? g : gmax;
    }
    return gmax;
}

// Host side of the exact weighted order statistics: an 8-bit radix select over the keys of ncols columns,
// nranks 0-based ranks (the same in every column, or one list per column), most significant digit first.  Per
// (rank, column) it holds the key prefix found so far and the rank left among the keys with that prefix.  A pass is
//   plan()      the distinct prefixes of each column's ranks ("groups", in order of first occurrence by rank):
//               group t of column c is slot gbase[c] + t, its prefix gpfx[slot]
//   (device)    digits[slot][256]: the weight of the column's keys with key >> (shift + 8) == gpfx[slot]
//               (every key in the first pass), by digit (key >> shift) & 255, added over all rows
//   advance()   walks each rank's histogram to its digit and extends the prefix
// until done(); key() is then the key of the order statistic.
struct RadixSelect {
    int ncols, nranks;
    int shift;                               // the digit of the coming pass; < 0: done
    int slots = 0, maxgroups = 0;            // of the last plan(): Σ ngroups, max ngroups
    std::vector<uint64_t> pfx, left;         // [nranks][ncols]
    std::vector<int> gbase, ngroups, slot;   // [ncols], [ncols], [nranks][ncols]
    std::vector<uint64_t> gpfx;              // [slots], room for nranks * ncols

    RadixSelect(int ncols_, int nranks_, int keybits, const uint64_t *ranks)
        : ncols(ncols_), nranks(nranks_), shift(keybits - 8), pfx((size_t)nranks_ * ncols_, 0),
          left((size_t)nranks_ * ncols_), gbase(ncols_), ngroups(ncols_), slot((size_t)nranks_ * ncols_),
          gpfx((size_t)nranks_ * ncols_)
    {
        for (int i = 0; i < nranks; i++)
            for (int c = 0; c < ncols; c++) left[(size_t)i * ncols + c] = ranks[i];
    }
    // ranks of its own for every column: ranks[nranks][ncols] (columns of sets with different weight totals).  The
    // library's handles all take this form, a single set included; both forms find the same exact order statistics.
    struct PerColumn {};
    RadixSelect(int ncols_, int nranks_, int keybits, const uint64_t *ranks, PerColumn)
        : RadixSelect(ncols_, nranks_, keybits, ranks)
    {
        for (size_t i = 0; i < left.size(); i++) left[i] = ranks[i];
    }
    bool done() const { return shift < 0; }
    void plan()
    {
        slots = maxgroups = 0;
        for (int c = 0; c < ncols; c++) {
            gbase[c] = slots;
            int n = 0;
            for (int i = 0; i < nranks; i++) {
                const uint64_t v = pfx[(size_t)i * ncols + c];
                int j = 0;
                while (j < n && gpfx[slots + j] != v) j++;
                if (j == n) gpfx[slots + n++] = v;
                slot[(size_t)i * ncols + c] = slots + j;
            }
            ngroups[c] = n;
            slots += n;
            maxgroups = n > maxgroups ? n : maxgroups;
        }
    }
    void advance(const uint64_t *digits)     // [slots][256] of the pass plan() prepared
    {
        for (size_t i = 0; i < pfx.size(); i++) {
            const uint64_t *h = digits + (size_t)slot[i] * 256;
            uint64_t cum = 0;
            int b = 0;
            for (; b < 255 && cum + h[b] <= left[i]; b++) cum += h[b];
            pfx[i] = (pfx[i] << 8) | (uint64_t)b;
            left[i] -= cum;
        }
        shift -= 8;
    }
    uint64_t key(int rank, int col) const { return pfx[(size_t)rank * ncols + col]; }
};

}  // namespace bh
