// posterior_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the per-row core of the posterior kernels (bayhunter_amd/csrc/posterior_core.h) with g++ so
// that the CPU tier replays the device arithmetic: Vs on the depth grid, interface depths, binning -- and the
// host side of the radix select (stats_core.h), which the test feeds with numpy's digit histograms.
#define BH_HOSTSIM 1
#include "../../bayhunter_amd/csrc/posterior_core.h"

template <typename T>
static void interp_rows(const T *rows, long R, int width, const double *dep, int D, double *vs, int *n,
                        double *ifd)
{
    for (long r = 0; r < R; r++) {
        const T *row = rows + r * width;
        const int c = bh::post_row_count(row, width);
        n[r] = c / 2;
        for (int k = 0; k < width / 2; k++) ifd[r * (width / 2) + k] = __builtin_nan("");
        if (c < 2) {
            for (int d = 0; d < D; d++) vs[r * D + d] = __builtin_nan("");
            continue;
        }
        bh::PostWalk<T> wi;
        wi.init(row, c);
        for (int k = 0; wi.has_interface(); k++) {
            ifd[r * (width / 2) + k] = wi.D;
            wi.cross();
        }
        bh::PostWalk<T> wk;
        wk.init(row, c);
        for (int d = 0; d < D; d++) vs[r * D + d] = (double)wk.at(dep[d]);
    }
}

extern "C" void ps_interp32(const float *rows, long R, int width, const double *dep, int D, double *vs, int *n,
                            double *ifd)
{
    interp_rows(rows, R, width, dep, D, vs, n, ifd);
}
extern "C" void ps_interp64(const double *rows, long R, int width, const double *dep, int D, double *vs, int *n,
                            double *ifd)
{
    interp_rows(rows, R, width, dep, D, vs, n, ifd);
}
extern "C" void ps_bin(const double *edges, int ne, const double *v, long nv, int *out)
{
    for (long i = 0; i < nv; i++) out[i] = bh::post_bin(edges, ne, v[i]);
}
extern "C" void ps_keys(const double *v, long nv, unsigned long long *k64, double *back)
{
    for (long i = 0; i < nv; i++) {
        k64[i] = bh::post_key64(v[i]);
        back[i] = bh::post_unkey64(k64[i]);
    }
}

// bh::RadixSelect: sel_new -> { sel_plan, <the caller counts digits[slots][256]>, sel_advance } until sel_plan
// returns a negative shift -> sel_keys
extern "C" void *ps_sel_new(int ncols, int nranks, int keybits, const uint64_t *ranks)
{
    return new bh::RadixSelect(ncols, nranks, keybits, ranks);
}
extern "C" void ps_sel_free(void *s) { delete (bh::RadixSelect *)s; }
// -> the digit's shift (< 0: done, nothing planned); gbase / ngroups [ncols], gpfx [nranks * ncols] (the first
// *slots are set), slot [nranks][ncols]
extern "C" int ps_sel_plan(void *s, int *gbase, int *ngroups, uint64_t *gpfx, int *slot, int *slots, int *maxgroups)
{
    bh::RadixSelect &r = *(bh::RadixSelect *)s;
    if (r.done()) return r.shift;
    r.plan();
    for (int c = 0; c < r.ncols; c++) { gbase[c] = r.gbase[c]; ngroups[c] = r.ngroups[c]; }
    for (int i = 0; i < r.slots; i++) gpfx[i] = r.gpfx[i];
    for (size_t i = 0; i < r.slot.size(); i++) slot[i] = r.slot[i];
    *slots = r.slots;
    *maxgroups = r.maxgroups;
    return r.shift;
}
extern "C" void ps_sel_advance(void *s, const uint64_t *digits) { ((bh::RadixSelect *)s)->advance(digits); }
extern "C" void ps_sel_keys(void *s, uint64_t *keys)                 // [nranks][ncols]
{
    bh::RadixSelect &r = *(bh::RadixSelect *)s;
    for (int i = 0; i < r.nranks; i++)
        for (int c = 0; c < r.ncols; c++) keys[(size_t)i * r.ncols + c] = r.key(i, c);
}
extern "C" void ps_keys32(const float *v, long nv, unsigned *k32, float *back)
{
    for (long i = 0; i < nv; i++) {
        k32[i] = bh::post_key32(v[i]);
        back[i] = bh::post_unkey32(k32[i]);
    }
}
