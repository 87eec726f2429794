// posterior_sets_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// The host side of the radix select (bayhunter_amd/csrc/stats_core.h) with one list of ranks per column, as the
// segmented posterior (posterior.hip) constructs it, compiled with g++; the test feeds it numpy's digit
// histograms.  per_column = 0 is the constructor every column shares one list with.
#define BH_HOSTSIM 1
#include "../../bayhunter_amd/csrc/stats_core.h"

// ranks: [nranks] (per_column = 0) or [nranks][ncols]
extern "C" void *pss_sel_new(int ncols, int nranks, int keybits, const uint64_t *ranks, int per_column)
{
    if (per_column) return new bh::RadixSelect(ncols, nranks, keybits, ranks, bh::RadixSelect::PerColumn());
    return new bh::RadixSelect(ncols, nranks, keybits, ranks);
}
extern "C" void pss_sel_free(void *s) { delete (bh::RadixSelect *)s; }
// -> the digit's shift (< 0: done, nothing planned); gbase / ngroups [ncols], gpfx [nranks * ncols] (the first
// *slots are set)
extern "C" int pss_sel_plan(void *s, int *gbase, int *ngroups, uint64_t *gpfx, int *slots)
{
    bh::RadixSelect &r = *(bh::RadixSelect *)s;
    if (r.done()) return r.shift;
    r.plan();
    for (int c = 0; c < r.ncols; c++) { gbase[c] = r.gbase[c]; ngroups[c] = r.ngroups[c]; }
    for (int i = 0; i < r.slots; i++) gpfx[i] = r.gpfx[i];
    *slots = r.slots;
    return r.shift;
}
extern "C" void pss_sel_advance(void *s, const uint64_t *digits) { ((bh::RadixSelect *)s)->advance(digits); }
extern "C" void pss_sel_keys(void *s, uint64_t *keys)                // [nranks][ncols]
{
    bh::RadixSelect &r = *(bh::RadixSelect *)s;
    for (int i = 0; i < r.nranks; i++)
        for (int c = 0; c < r.ncols; c++) keys[(size_t)i * r.ncols + c] = r.key(i, c);
}
extern "C" void pss_keys64(const double *v, long nv, unsigned long long *k)
{
    for (long i = 0; i < nv; i++) k[i] = bh::post_key64(v[i]);
}
extern "C" void pss_keys32(const float *v, long nv, unsigned *k)
{
    for (long i = 0; i < nv; i++) k[i] = bh::post_key32(v[i]);
}
