// pairs_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the core of the segmented joint histograms (bayhunter_amd/csrc/pairs_core.h) with g++ so that the CPU tier
// replays the kernel's steps -- slots, the LDS plan, blocks of a set, groups of pairs, the per-row step -- against the
// numpy restatement (tests/scalars_ref.py).
#define BH_HOSTSIM 1
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/pairs_core.h"

namespace {
struct PlainAdd {
    void operator()(uint64_t *cell, uint64_t wt) const { *cell += wt; }
};
}  // namespace

// the dynamic LDS bytes of a block and the pairs per group, as the library plans them
extern "C" long ps_plan(int nslots, int nedges, int npairs, int *group)
{
    return (long)bh::pairs_plan(nslots, nedges, npairs, group);
}

extern "C" int ps_static_lds(void) { return bh::kPairsStaticLds; }

// bh_hist2d_sets as its kernel walks it: a block per stretch of rows_per_block rows of a set, the pairs in groups of
// `group` (0: the library's plan), one table per group as the block's LDS holds it, flushed into hist.
// -> 0, or 1 for a negative weight
extern "C" int ps_hist2d_sets(const double *D, long long nrows, long long stride, int ncols, const int *weights,
                              const long long *set_start, int nsets, const int *pairs, int npairs, const double *edges,
                              int nedges, long long *hist, int group, long long rows_per_block)
{
    (void)nrows;
    int slot_col[2 * BH_PAIRS_MAX];
    bh::PairCols tab[BH_PAIRS_MAX];
    const int nslots = bh::pairs_slots(pairs, npairs, slot_col, tab);
    const size_t ne = (size_t)nedges, nb = ne - 1;
    if (group < 1) bh::pairs_plan(nslots, nedges, npairs, &group);
    std::vector<double> ed((size_t)nslots * ne);
    std::vector<uint64_t> lds((size_t)group * nb * nb);
    int negative = 0;
    std::memset(hist, 0, sizeof(long long) * (size_t)nsets * npairs * nb * nb);
    for (int z = 0; z < nsets; z++) {
        for (int s = 0; s < nslots; s++)
            std::memcpy(&ed[(size_t)s * ne], edges + ((size_t)z * ncols + slot_col[s]) * ne, sizeof(double) * ne);
        for (long long r0 = set_start[z]; r0 < set_start[z + 1]; r0 += rows_per_block) {
            const long long r1 = r0 + rows_per_block < set_start[z + 1] ? r0 + rows_per_block : set_start[z + 1];
            for (int p0 = 0; p0 < npairs; p0 += group) {
                const int np = npairs - p0 < group ? npairs - p0 : group;
                std::fill(lds.begin(), lds.end(), 0);
                for (long long r = r0; r < r1; r++) {
                    const int wt = weights ? weights[r] : 1;
                    if (wt < 0 && p0 == 0) negative = 1;
                    if (wt <= 0) continue;
                    bh::pairs_row(D + r * stride, tab + p0, np, ed.data(), nedges, (uint64_t)wt, lds.data(), PlainAdd());
                }
                long long *out = hist + ((size_t)z * npairs + p0) * nb * nb;
                for (size_t i = 0; i < (size_t)np * nb * nb; i++) out[i] += (long long)lds[i];
            }
        }
    }
    return negative;
}
