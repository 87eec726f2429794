// pairs_core.h -- the bin rule, the per-row step and the LDS plan of the segmented joint histograms (pairs.hip,
// bh_hist2d_sets).
//
// A pair is two columns (x, y) of a row of doubles.  Every set of rows has its own ascending edges per column; a row of
// weight w adds w to the cell (bx, by) of each pair whose two values both fall inside their edges -- numpy's rule, as
// np.histogram2d applies it per axis: e[i] <= v < e[i+1], the last bin closed (post_bin, stats_core.h).  A NaN falls
// outside every bin, so it takes the row out of the pairs that read its column and out of no other.
//
// A block keeps the edges of the columns its pairs name ("slots": the distinct columns, 2 * BH_PAIRS_MAX at most) and
// the u64 cell tables of as many pairs as fit beside them in LDS; pairs_plan() is that split.  The counts are integer
// sums: neither the split nor the order of the rows changes them.
// Compiled with g++ under BH_HOSTSIM by tests/hostsim/pairs_sim.cpp (test infrastructure only).
#pragma once
#include "../../include/bayhunter_amd.h"      // BH_PAIRS_MAX, BH_PAIRS_MAX_EDGES
#include "bh_common.h"
#include "stats_core.h"

namespace bh {

constexpr int kPairsLdsBytes = 64 * 1024;       // a block's LDS, static part included
constexpr int kPairsStaticLds = 4 * BH_PAIRS_MAX * (int)sizeof(int);    // the pair table of pairs.hip

// one pair of the block's table: the two columns of the row, and the slots of their edges
struct PairCols { int cx, cy, ex, ey; };

// the distinct columns of pairs[npairs][2] in order of first use -> their number; slot_col[slot] is the column,
// tab[p] the pair with its slots
inline int pairs_slots(const int *pairs, int npairs, int *slot_col, PairCols *tab)
{
    int nu = 0;
    for (int p = 0; p < npairs; p++) {
        int s[2];
        for (int k = 0; k < 2; k++) {
            const int c = pairs[2 * p + k];
            int j = 0;
            while (j < nu && slot_col[j] != c) j++;
            if (j == nu) slot_col[nu++] = c;
            s[k] = j;
        }
        tab[p].cx = pairs[2 * p];
        tab[p].cy = pairs[2 * p + 1];
        tab[p].ex = s[0];
        tab[p].ey = s[1];
    }
    return nu;
}

// How a block's dynamic LDS is split: nslots * nedges doubles of edges, then the cell tables of `group` pairs
// (nb * nb u64 each) -> the dynamic bytes; *group >= 1 for every nslots <= 2 * BH_PAIRS_MAX, nedges <= 65.
inline size_t pairs_plan(int nslots, int nedges, int npairs, int *group)
{
    const size_t nb = (size_t)(nedges - 1);
    const size_t ebytes = sizeof(double) * (size_t)nslots * (size_t)nedges;
    const size_t room = (size_t)(kPairsLdsBytes - kPairsStaticLds) - ebytes;
    size_t g = room / (nb * nb * sizeof(uint64_t));
    if (g > (size_t)npairs) g = (size_t)npairs;
    *group = (int)g;
    return ebytes + g * nb * nb * sizeof(uint64_t);
}

// The cell of (x, y) among the edges ex[ne], ey[ne]: bx * nb + by, or -1 when either value is a NaN or outside.
BH_HD int pairs_cell(const double *ex, const double *ey, int ne, double x, double y)
{
    const int bx = post_bin(ex, ne, x);
    if (bx < 0) return -1;
    const int by = post_bin(ey, ne, y);
    if (by < 0) return -1;
    return bx * (ne - 1) + by;
}

// One row `d` of weight wt > 0 into the tables tab[np][nb * nb] of the pairs pr[0 .. np): edges[slot][ne] are the
// set's.  `add(&cell, wt)` is the atomic add of the block on the device, a plain one in the host build.
template <typename Add>
BH_HD void pairs_row(const double *d, const PairCols *pr, int np, const double *edges, int ne, uint64_t wt,
                     uint64_t *tab, Add add)
{
    const int nb = ne - 1;
    for (int p = 0; p < np; p++) {
        const int cell = pairs_cell(edges + pr[p].ex * ne, edges + pr[p].ey * ne, ne, d[pr[p].cx], d[pr[p].cy]);
        if (cell >= 0) add(tab + (size_t)p * nb * nb + cell, wt);
    }
}

}  // namespace bh
