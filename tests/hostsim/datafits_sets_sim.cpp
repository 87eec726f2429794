// datafits_sets_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// The part of bayhunter_amd/csrc/datafits_kernel.h that needs no device, compiled with g++: the number of blocks along
// the rows of a set (what makes a set of the segmented form the grid of a single handle) and the number of sets a
// chunk of the radix select takes.  The block body itself (df_block) is device code and is compared on the GPU
// (tests/test_gpu_datafits_sets.py).
// With it the slab offsets of the segmented reductions (stats_core.h: set_slab_offsets) over either file's blocks_of:
// posterior_kernel.h has the posterior's above its own fence.
#define BH_HOSTSIM 1
#include "../../bayhunter_amd/csrc/datafits_kernel.h"
#include "../../bayhunter_amd/csrc/posterior_kernel.h"

extern "C" int dfs_blocks_of(long long nrows) { return bh::fit::blocks_of(nrows); }
extern "C" int pos_blocks_of(long long nrows) { return bh::post::blocks_of(nrows); }
// goff[nsets + 1] as SetStats::alloc_sets fills it for bh_posterior_sets (posterior != 0) or bh_datafits_sets -> Gmax
extern "C" int sets_slab_offsets(int posterior, const long long *start, int nsets, long long *goff)
{
    return bh::set_slab_offsets(start, nsets, posterior ? bh::post::blocks_of : bh::fit::blocks_of, goff);
}
extern "C" int dfs_sets_per_chunk(int nsets, int ncols, int nranks, int gz, long long bytes)
{
    return bh::fit::sets_per_chunk(nsets, ncols, nranks, gz, bytes);
}
// the chunks bh_datafits_sets_finish walks: first[i] .. first[i + 1] -> number of chunks
extern "C" int dfs_chunks(int nsets, int ncols, int nranks, long long bytes, int *first)
{
    const int gz = (nranks + bh::fit::kGroups - 1) / bh::fit::kGroups;
    const int chunk = bh::fit::sets_per_chunk(nsets, ncols, nranks, gz, bytes);
    int n = 0;
    for (int f = 0; f < nsets; f += chunk) first[n++] = f;
    first[n] = nsets;
    return n;
}
