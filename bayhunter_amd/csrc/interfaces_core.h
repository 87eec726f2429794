// interfaces_core.h -- per-row arithmetic of the discontinuity statistics (interfaces.hip).
//
// A row is a model in the reference's layout [vs(n), z_vnoi(n), NaN...] (src/Models.py:16-24) in float32 or float64
// with an integer weight w.  Its interfaces k = 0 .. n-2 lie at the depths D_k of PostWalk (posterior_core.h: z_disc
// midpoints, the sequential fp64 cumsum) and carry the jump J_k = (double)vs[k+1] - (double)vs[k].  With d the bin of
// D_k among the depth edges and j the bin of J_k among the jump edges (post_bin: numpy's rule, -1 outside), an
// interface with d >= 0 adds w to the cells of depth bin d:
//
//   IF_COUNT                       every interface
//   IF_NEG / IF_POS                J < 0 / J > 0 (J == 0 and a NaN are neither)
//   IF_MODELS / _NEG / _POS        once per run of consecutive interfaces of the row in bin d (with such a jump): the
//                                  walk keeps (last bin, seen, seen_neg, seen_pos) and starts anew when the bin changes,
//                                  so for a depth-sorted row this counts models, not interfaces
//   IF_FIELDS + j                  the joint histogram, j >= 0 only
//
// An interface with d < 0 adds nothing and leaves the run as it is.  The cells of a depth bin lie together
// ([depth bin][IF_FIELDS + jump bins]) so that a kernel may hold a range [d0, d1) of depth bins in LDS; the walk then
// emits the cells of that range only, and the runs are still followed over all bins.
//
// The two floating-point sums Σ w·J and Σ w·(J - mean_d)² take an order the row alone cannot give: interfaces_order()
// below states it once, for the kernel and for the host twin.  Compiled with g++ under BH_HOSTSIM by
// tests/hostsim/interfaces_sim.cpp (test infrastructure only).
#pragma once
#include "bh_common.h"
#include "posterior_core.h"

namespace bh {

enum { IF_COUNT = 0, IF_MODELS, IF_NEG, IF_POS, IF_MODELS_NEG, IF_MODELS_POS, IF_FIELDS };

constexpr int kIfThreads = 256;                     // rows of a trip: one per thread
constexpr int kIfWave = 64;
constexpr int kIfWaves = kIfThreads / kIfWave;
constexpr int kIfTrips = 8;
constexpr int kIfRowsPerBlock = kIfTrips * kIfThreads;   // a block's stretch of its set
constexpr int kIfLdsBytes = 60 * 1024;              // the dynamic LDS a block may take for its cells

// blocks of a set of nrows rows: a function of the row count alone (an empty set has none)
inline int interfaces_blocks_of(long long nrows)
{
    return (int)((nrows + kIfRowsPerBlock - 1) / kIfRowsPerBlock);
}

// depth bins whose cells fit kIfLdsBytes together: the kernel takes the bins in groups of this many
inline int interfaces_group(int nbd, int nbj)
{
    const int g = kIfLdsBytes / (8 * (IF_FIELDS + nbj));
    return g < nbd ? g : nbd;
}

// The jump of interface wk.k (the walk stands above it: wk.has_interface()).
template <typename T>
BH_POST_M double interfaces_jump(const PostWalk<T> &wk)
{
    return (double)wk.row[wk.k + 1] - (double)wk.row[wk.k];
}

// The integer cells of one row: add(cell, w) for every cell of the depth bins [d0, d1), cell = (d - d0) * (IF_FIELDS +
// nbj) + field.  jedges may be NULL (nje 0): no joint histogram.
template <typename T, typename Add>
BH_POST_M void interfaces_row(const T *row, int width, uint64_t w, const double *dedges, int nde, const double *jedges,
                              int nje, int d0, int d1, uint64_t *tab, Add add)
{
    const int c = post_row_count(row, width);
    if (c < 4) return;                              // fewer than two nuclei: no interface
    const int cells = IF_FIELDS + (nje > 1 ? nje - 1 : 0);
    PostWalk<T> wk;
    wk.init(row, c);
    int last = -1;
    bool seen = false, seen_neg = false, seen_pos = false;
    while (wk.has_interface()) {
        const int d = post_bin(dedges, nde, wk.D);
        if (d >= 0) {
            const double J = interfaces_jump(wk);
            if (d != last) {
                last = d;
                seen = seen_neg = seen_pos = false;
            }
            if (d >= d0 && d < d1) {
                uint64_t *cell = tab + (size_t)(d - d0) * cells;
                add(cell + IF_COUNT, w);
                if (!seen) add(cell + IF_MODELS, w);
                if (J < 0.0) {
                    add(cell + IF_NEG, w);
                    if (!seen_neg) add(cell + IF_MODELS_NEG, w);
                } else if (J > 0.0) {
                    add(cell + IF_POS, w);
                    if (!seen_pos) add(cell + IF_MODELS_POS, w);
                }
                if (nje > 1) {
                    const int j = post_bin(jedges, nje, J);
                    if (j >= 0) add(cell + IF_FIELDS + j, w);
                }
            }
            seen = true;
            seen_neg = seen_neg || J < 0.0;
            seen_pos = seen_pos || J > 0.0;
        }
        wk.cross();
    }
}

// What interface k of a row adds to a floating-point sum of depth bin d: w·J, or w·(J - mean[d])² with `mean`.
BH_HD double interfaces_term(double w, double J, const double *mean, int d)
{
    if (!mean) return w * J;
    const double e = J - mean[d];
    return w * (e * e);
}

// The order of the floating-point sums (interfaces_order):
//   a set's rows are cut into blocks of kIfRowsPerBlock rows from the set's first row; in a block, row i belongs to
//   trip i / kIfThreads, wave (i % kIfThreads) / kIfWave, lane i % kIfWave.  A wave keeps one accumulator per depth bin,
//   0.0 at first, and adds its terms trip after trip, in a trip interface index k ascending, for one k the lanes
//   ascending.  A block's partial is ((wave 0 + wave 1) + wave 2) + wave 3, a set's sum 0.0 plus its blocks' partials
//   in block order.  Nothing in it depends on where the set lies or on the other sets.

}  // namespace bh
