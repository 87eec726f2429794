// posterior.hip -- velocity-depth posterior statistics of a block of sampled models (bh_posterior_*).
//
// The reference reaches the posterior through ModelMatrix.get_singlemodels (src/Models.py:160-226) and
// PlotFromStorage._plot_bestmodels_hist (src/Plotting.py:462-536): every model interpolated onto a depth
// grid in a Python loop, rows repeated once per iteration they stayed current.  Here every row carries an
// integer weight and is walked on the device (posterior_core.h); nothing is expanded.  The depths are the
// columns of the weighted column reduction whose shared parts are in stats_core.h / stats_host.h (keys, slabs,
// the scan / finish hand-over, the radix select); this file has what is the posterior's own:
//
//   the walk   a thread per row, kTile depths of the ascending grid per block in registers
//   scan       besides the columns' min / max / Σ w·v, per row (blocks of the first depth tile only): the
//              weight total, the layer-count histogram, the interface-depth histogram, the first argmin of
//              the misfit
//   finish     Σ w·(v - mean)², one 2-D (depth bin, Vs bin) histogram over edges the caller computed, and the
//              median: the select's two middle ranks, over 32-bit keys for float32 rows (4 passes) and 64-bit
//              for float64; the first digit pass shares the row walk with the sums and the histogram
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include "host_common.h"
#include "posterior_kernel.h"

namespace {

using bh::u64;
using namespace bh::post;

template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void post_kernel(PostArgs a)
{
    post_block<T, MODE>(a, 0, a.nrows, (int)blockIdx.x, (int)gridDim.x);
}

}  // namespace


struct bh_posterior : bh::ColumnStats {          // n: the depths
    int fp64 = 0, width = 0, nif = 0, maxn = 0;
    const void *rows = nullptr;
    long long nrows = 0, stride = 0;
    const int *w = nullptr;
    const double *misfit = nullptr;
    // device
    double *dep = nullptr, *ifedges = nullptr;
    u64 *cnt = nullptr, *nlay = nullptr, *ifhist = nullptr, *mfkey = nullptr;
    long long *mfrow = nullptr;
};

namespace {

template <typename T, int MODE>
int launch(bh_posterior *p, PostArgs &a, size_t lds_bytes)
{
    dim3 grid((unsigned)p->G, (unsigned)((p->n + kTile - 1) / kTile));
    hipLaunchKernelGGL((post_kernel<T, MODE>), grid, dim3(kThreads), lds_bytes, p->st, a);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

template <int MODE>
int run(bh_posterior *p, PostArgs &a, size_t lds_bytes)
{
    return p->fp64 ? launch<double, MODE>(p, a, lds_bytes) : launch<float, MODE>(p, a, lds_bytes);
}

PostArgs base_args(const bh_posterior *p)
{
    PostArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = p->rows;
    a.nrows = p->nrows;
    a.stride = p->stride;
    a.width = p->width;
    a.D = p->n;
    a.w = p->w;
    a.misfit = p->misfit;
    a.dep = p->dep;
    a.slab = p->slab;
    a.maxn = p->maxn;
    return a;
}

}  // namespace

extern "C" {

int bh_posterior_create(const void *rows, int fp64, long long nrows, long long stride, int width,
                        const int *weights, const double *misfits, const double *dep, int ndep,
                        const double *ifedges, int nifedges, void *stream, bh_posterior **post)
{
    if (!post) return bh::fail_arg_("post is NULL");
    *post = nullptr;
    if (!rows || nrows < 1) return bh::fail_arg_("bh_posterior_create: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_posterior_create: more than 2^32 rows (the weight total could overflow)");
    if (width < 2 || width > 2 * BH_MAX_LAYERS + 2 || stride < width) return bh::fail_arg_("bh_posterior_create: width / stride");
    if (!dep || ndep < 1 || !bh::ascending(dep, ndep)) return bh::fail_arg_("bh_posterior_create: the depth grid must be ascending");
    if (nifedges && (nifedges < 2 || !ifedges || !bh::ascending(ifedges, nifedges)))
        return bh::fail_arg_("bh_posterior_create: interface edges must be ascending");
    if (int rc = bh::require_device()) return rc;
    std::unique_ptr<bh_posterior> p(new (std::nothrow) bh_posterior);
    if (!p) return bh::fail_arg_("out of memory");
    p->fp64 = fp64 ? 1 : 0;
    p->rows = rows;
    p->nrows = nrows;
    p->stride = stride;
    p->width = width;
    p->w = weights;
    p->misfit = misfits;
    p->n = ndep;
    p->nif = nifedges;
    p->maxn = width / 2;
    p->st = (hipStream_t)stream;
    p->G = blocks_of(nrows);
    int rc = p->alloc_columns();
    if (rc) return rc;
    BH_HIP(p->bufs.alloc(p->dep, ndep));
    BH_HIP(p->bufs.alloc(p->cnt, 2));
    BH_HIP(p->bufs.alloc(p->nlay, p->maxn + 1));
    BH_HIP(p->bufs.alloc(p->mfkey, p->G));
    BH_HIP(p->bufs.alloc(p->mfrow, p->G));
    BH_HIP(hipMemcpyAsync(p->dep, dep, sizeof(double) * ndep, hipMemcpyHostToDevice, p->st));
    if (nifedges) {
        BH_HIP(p->bufs.alloc(p->ifedges, nifedges));
        BH_HIP(p->bufs.alloc(p->ifhist, nifedges - 1));
        BH_HIP(hipMemcpyAsync(p->ifedges, ifedges, sizeof(double) * nifedges, hipMemcpyHostToDevice, p->st));
    }
    BH_HIP(hipStreamSynchronize(p->st));
    *post = p.release();
    return BH_OK;
}

void bh_posterior_destroy(bh_posterior *post)
{
    if (post) {
        (void)hipStreamSynchronize(post->st);
        delete post;
    }
}

int bh_posterior_scan(bh_posterior *p, long long *total, double *vmin, double *vmax, double *mean,
                      long long *nlayers, long long *ifhist, long long *argmin)
{
    if (!p) return bh::fail_arg_("post is NULL");
    int rc = p->begin_scan();
    if (rc) return rc;
    BH_HIP(hipMemsetAsync(p->cnt, 0, sizeof(u64) * 2, p->st));
    BH_HIP(hipMemsetAsync(p->nlay, 0, sizeof(u64) * (p->maxn + 1), p->st));
    if (p->nif) BH_HIP(hipMemsetAsync(p->ifhist, 0, sizeof(u64) * (p->nif - 1), p->st));
    PostArgs a = base_args(p);
    a.flags = F_ROWS;
    a.kmin = p->kmin;
    a.kmax = p->kmax;
    a.cnt = p->cnt;
    a.nlay = p->nlay;
    a.ifedges = p->ifedges;
    a.nif = p->nif;
    a.ifhist = p->ifhist;
    a.mfkey = p->mfkey;
    a.mfrow = p->mfrow;
    a.off_nlay = 0;
    a.off_if = p->maxn + 1;
    const size_t lds = sizeof(u64) * (size_t)(p->maxn + 1 + (p->nif > 1 ? p->nif - 1 : 0));
    rc = run<MODE_SCAN>(p, a, lds);
    if (rc) return rc;
    u64 cnt[2];                                    // weight total, rows with a negative weight
    std::vector<u64> nl(p->maxn + 1), ih(p->nif > 1 ? p->nif - 1 : 0), mk(p->G);
    std::vector<long long> mr(p->G);
    BH_HIP(hipMemcpyAsync(cnt, p->cnt, sizeof(cnt), hipMemcpyDeviceToHost, p->st));
    BH_HIP(hipMemcpyAsync(nl.data(), p->nlay, sizeof(u64) * nl.size(), hipMemcpyDeviceToHost, p->st));
    if (!ih.empty()) BH_HIP(hipMemcpyAsync(ih.data(), p->ifhist, sizeof(u64) * ih.size(), hipMemcpyDeviceToHost, p->st));
    if (p->misfit) {
        BH_HIP(hipMemcpyAsync(mk.data(), p->mfkey, sizeof(u64) * p->G, hipMemcpyDeviceToHost, p->st));
        BH_HIP(hipMemcpyAsync(mr.data(), p->mfrow, sizeof(long long) * p->G, hipMemcpyDeviceToHost, p->st));
    }
    std::vector<double> sum;
    rc = p->reduce_slab(sum);                      // synchronises the stream
    if (!rc) rc = p->end_scan("bh_posterior_scan", cnt[0], cnt[1], sum, vmin, vmax, mean);
    if (rc) return rc;
    if (total) *total = (long long)p->total;
    if (nlayers)
        for (size_t i = 0; i < nl.size(); i++) nlayers[i] = (long long)nl[i];
    if (ifhist)
        for (size_t i = 0; i < ih.size(); i++) ifhist[i] = (long long)ih[i];
    if (argmin) {
        long long best = -1;
        u64 bk = 0;
        for (int g = 0; p->misfit && g < p->G; g++)
            if (mr[g] >= 0 && (best < 0 || mk[g] < bk || (mk[g] == bk && mr[g] < best))) { best = mr[g]; bk = mk[g]; }
        *argmin = best;
    }
    return BH_OK;
}

int bh_posterior_finish(bh_posterior *p, const double *vedges, int nvedges, const int *dbin, int ndbins,
                        long long *hist, double *stdev, double *median)
{
    if (!p) return bh::fail_arg_("post is NULL");
    if (!p->scanned) return bh::fail_arg_("bh_posterior_finish before bh_posterior_scan");
    const int D = p->n;
    const bool want_hist = vedges != nullptr;
    if (want_hist && (nvedges < 2 || !bh::ascending(vedges, nvedges) || !dbin || ndbins < 1 || !hist))
        return bh::fail_arg_("bh_posterior_finish: Vs edges must be ascending, depth bins and histogram given");
    const int tile_fits = want_hist ? tiles_fit(dbin, D, ndbins) : 1;
    if (tile_fits < 0) return bh::fail_arg_("bh_posterior_finish: depth bin out of range");
    const int nvb = nvedges - 1;
    bh::DevBufs tmp;
    PostArgs a = base_args(p);
    a.mean = p->dmean;
    if (want_hist) {
        double *dve = nullptr;
        int *ddb = nullptr;
        BH_HIP(tmp.alloc(dve, nvedges));
        BH_HIP(tmp.alloc(ddb, D));
        BH_HIP(tmp.alloc(a.hist, (size_t)ndbins * nvb));
        BH_HIP(hipMemcpyAsync(dve, vedges, sizeof(double) * nvedges, hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemcpyAsync(ddb, dbin, sizeof(int) * D, hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemsetAsync(a.hist, 0, sizeof(u64) * (size_t)ndbins * nvb, p->st));
        a.flags |= F_HIST;
        a.vedges = dve;
        a.nve = nvedges;
        a.dbin = ddb;
        a.ndb = ndbins;
        if (!tile_fits || (size_t)kTile * nvb * sizeof(u64) > (size_t)kHistLdsBytes) a.flags |= F_HIST_GLOBAL;
    }
    // the median: the select's ranks are the two middle order statistics (0-based), at most two groups a depth
    const uint64_t mid[2] = {(p->total - 1) / 2, p->total / 2};
    bh::DeviceSelect sel(D, median ? 2 : 0, p->fp64 ? 64 : 32, mid);
    if (median) {
        int rc = sel.alloc(tmp);
        if (rc) return rc;
        a.flags |= F_RADIX;
        a.gbase = sel.dgbase;
        a.ngroups = sel.dngroups;
        a.gpfx = sel.dgpfx;
        a.digits = sel.ddigits;
    }
    if (stdev) a.flags |= F_SQ;
    // LDS: radix digits first, then the histogram tile
    a.off_radix = 0;
    a.off_hist = median ? kTile * 2 * 256 : 0;
    size_t lds = sizeof(u64) * (size_t)(a.off_hist + ((a.flags & F_HIST) && !(a.flags & F_HIST_GLOBAL) ? kTile * nvb : 0));
    for (bool first = true; first || (median && !sel.done()); first = false) {
        int rc = median ? sel.begin_pass(p->st) : BH_OK;
        a.shift = median ? sel.shift : 0;
        if (!rc) rc = run<MODE_FINISH>(p, a, lds);
        if (!rc && first && stdev) rc = p->read_stdev(stdev);
        if (!rc && first && want_hist) rc = bh::read_hist(a.hist, (size_t)ndbins * nvb, hist, p->st);
        if (rc) return rc;
        a.flags &= ~(F_SQ | F_HIST | F_HIST_GLOBAL);   // later passes: digits only
        lds = sizeof(u64) * (size_t)(kTile * 2 * 256);
        if (!median) break;
        rc = sel.end_pass(p->st);
        if (rc) return rc;
    }
    if (median)
        for (int d = 0; d < D; d++) median[d] = median_of(sel, p->fp64, d);
    return BH_OK;
}

}  // extern "C"
