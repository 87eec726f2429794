// posterior.hip -- velocity-depth posterior statistics of a block of sampled models: of many sets of rows at once
// (bh_posterior_sets_*) and of all rows as one set (bh_posterior_*).
//
// The reference reaches the posterior through ModelMatrix.get_singlemodels (src/Models.py:160-226) and
// PlotFromStorage._plot_bestmodels_hist (src/Plotting.py:462-536): every model interpolated onto a depth
// grid in a Python loop, rows repeated once per iteration they stayed current.  Here every row carries an
// integer weight and is walked on the device (posterior_core.h); nothing is expanded.  The depths are the
// columns of the weighted column reduction whose shared parts are in stats_core.h / stats_host.h (keys, slabs,
// the scan / finish hand-over, the radix select); this file has what is the posterior's own:
//
//   the walk   a thread per row, kTile depths of the ascending grid per block in registers (posterior_kernel.h)
//   scan       besides the columns' min / max / Σ w·v, per row (blocks of the first depth tile only): the
//              weight total, the layer-count histogram, the interface-depth histogram, the first argmin of
//              the misfit
//   finish     Σ w·(v - mean)², one 2-D (depth bin, Vs bin) histogram over edges the caller computed, and the
//              median: the select's two middle ranks, over 32-bit keys for float32 rows (4 passes) and 64-bit
//              for float64; the first digit pass shares the row walk with the sums and the histogram
//
// A network inverted in one pool (StationPool) is read station by station, and one handle per station would be a few
// thousand rows per launch, i.e. the latency of its launches, copies and synchronisations times the number of
// stations.  So the rows come in contiguous segments, one per set, and a block belongs to one set: blockIdx.z names
// it, and the block walks the set's rows as block x of the G blocks of a set of that many rows, with the set's own
// outputs.  The slab of a set is added in block order, and the mean and the standard deviation leave the host through
// one expression each: no number of a set depends on the set's offset, on its neighbours or on the chunking, and a
// bh_posterior handle is the sets handle with the single set [0, nrows) (the wrappers at the end of the file).
//
//   scan     one launch (grid: blocks of the largest set, depth tiles, sets) and one slab reduction
//   slab     the sets' partials one after the other, set z owning G(z) rows from goff[z] (stats_host.h: SetStats)
//   finish   per set its own Vs edges (concatenated, with offsets) and histogram; the select runs over
//            nsets * D columns with each set's two middle ranks; one launch per radix pass for all sets
//   chunks   the select's digit table is 2 * 256 * 8 B per column, so the finish takes the sets in chunks whose
//            table stays under a budget; a set is never split, and nothing a set's blocks compute depends on the chunk
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include "host_common.h"
#include "posterior_kernel.h"

namespace {

using bh::u64;
using namespace bh::post;

constexpr long long kDigitBudget = 64ll << 20;       // bytes of digit table per chunk (bh_posterior_sets_set_chunk_bytes)

enum { S_SKIP = bh::SET_SKIP, S_HIST_GLOBAL = 2 };   // per set, for the finish

struct SetArgs {
    const long long *start;            // [nsets + 1] rows of set z: start[z] .. start[z + 1]
    const long long *goff;             // [nsets + 1] slab rows (and argmin partials) before set z
    int first;                         // the launch's first set
    const int *sflags;                 // [nsets] finish: S_SKIP, S_HIST_GLOBAL
    const int *vedge_off;              // [nsets + 1] into vedges
    const u64 *hist_off;               // [nsets + 1] into hist
};

template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void post_sets_kernel(PostArgs a, SetArgs s)
{
    const int zl = blockIdx.z, z = s.first + zl;
    const long long r0 = s.start[z], r1 = s.start[z + 1];
    const int G = blocks_of(r1 - r0), bx = blockIdx.x;
    if (bx >= G) return;
    const size_t col = (size_t)z * a.D;
    a.slab += (size_t)s.goff[z] * a.D;
    if (MODE == MODE_SCAN) {
        a.kmin += col;
        a.kmax += col;
        a.cnt += 2 * (size_t)z;
        a.nlay += (size_t)z * (a.maxn + 1);
        if (a.nif > 1) a.ifhist += (size_t)z * (a.nif - 1);
        a.mfkey += s.goff[z];
        a.mfrow += s.goff[z];
    } else {
        const int f = s.sflags[z];
        if (f & S_SKIP) return;
        a.mean += col;
        if (a.flags & F_HIST) {
            a.vedges += s.vedge_off[z];
            a.nve = s.vedge_off[z + 1] - s.vedge_off[z];
            a.hist += s.hist_off[z];
            if (f & S_HIST_GLOBAL) a.flags |= F_HIST_GLOBAL;
        }
        if (a.flags & F_RADIX) {
            a.gbase += (size_t)zl * a.D;
            a.ngroups += (size_t)zl * a.D;
        }
    }
    post_block<T, MODE>(a, r0, r1, bx, G);
}

}  // namespace

struct bh_posterior_sets : bh::SetStats<blocks_of> {
    int fp64 = 0, width = 0, nif = 0, maxn = 0;          // n of SetStats: the depths
    long long chunk_bytes = 0;
    const void *rows = nullptr;
    long long nrows = 0, stride = 0;
    const int *w = nullptr;
    const double *misfit = nullptr;
    // device
    double *dep = nullptr, *ifedges = nullptr;
    u64 *cnt = nullptr, *nlay = nullptr, *ifhist = nullptr, *mfkey = nullptr;    // [nsets][2], ..., [goff[nsets]]
    long long *mfrow = nullptr;
};

struct bh_posterior : bh_posterior_sets {};              // all rows as the one set of the handle

namespace {

template <typename T, int MODE>
int launch(bh_posterior_sets *p, PostArgs &a, SetArgs &s, int nc, size_t lds_bytes)
{
    dim3 grid((unsigned)p->chunk_blocks(s.first, nc), (unsigned)((p->n + kTile - 1) / kTile), (unsigned)nc);
    hipLaunchKernelGGL((post_sets_kernel<T, MODE>), grid, dim3(kThreads), lds_bytes, p->st, a, s);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

template <int MODE>
int run(bh_posterior_sets *p, PostArgs &a, SetArgs &s, int nc, size_t lds_bytes)
{
    return p->fp64 ? launch<double, MODE>(p, a, s, nc, lds_bytes) : launch<float, MODE>(p, a, s, nc, lds_bytes);
}

PostArgs base_args(const bh_posterior_sets *p)
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

SetArgs set_args(const bh_posterior_sets *p)
{
    SetArgs s;
    std::memset(&s, 0, sizeof(s));
    s.start = p->dstart;
    s.goff = p->dgoff;
    s.sflags = p->dskip;
    return s;
}

template <typename T>
int fetch(std::vector<T> &host, const T *dev, size_t count, hipStream_t st)
{
    host.resize(count);
    if (count) BH_HIP(hipMemcpyAsync(host.data(), dev, sizeof(T) * count, hipMemcpyDeviceToHost, st));
    return BH_OK;
}

// ---- the three steps of a handle; `who` is the entry point that reports what they refuse ------------------------

// the arguments, then the fresh handle `p` (NULL: there was no memory for it) with its device buffers
int create(const char *who, bh_posterior_sets *p, const void *rows, int fp64, long long nrows, long long stride,
           int width, const int *weights, const double *misfits, const long long *set_start, int nsets,
           const double *dep, int ndep, const double *ifedges, int nifedges, void *stream)
{
    if (!rows || nrows < 1) return bh::fail_who(who, "no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_who(who, "more than 2^32 rows (the weight total could overflow)");
    if (width < 2 || width > 2 * BH_MAX_LAYERS + 2 || stride < width) return bh::fail_who(who, "width / stride");
    if (nsets < 1 || nsets > 65535) return bh::fail_who(who, "1 to 65535 sets");
    if (int rc = bh::check_set_start(who, set_start, nsets, nrows)) return rc;
    if (!dep || ndep < 1 || !bh::ascending(dep, ndep)) return bh::fail_who(who, "the depth grid must be ascending");
    if ((long long)nsets * ndep > 0x3fffffff) return bh::fail_who(who, "more than 2^30 (set, depth) columns");
    if (nifedges && (nifedges < 2 || !ifedges || !bh::ascending(ifedges, nifedges)))
        return bh::fail_who(who, "interface edges must be ascending");
    if (int rc = bh::require_device()) return rc;
    if (!p) return bh::fail_arg_("out of memory");
    p->fp64 = fp64 ? 1 : 0;
    p->rows = rows;
    p->nrows = nrows;
    p->stride = stride;
    p->width = width;
    p->w = weights;
    p->misfit = misfits;
    p->n = ndep;
    p->nsets = nsets;
    p->nif = nifedges;
    p->maxn = width / 2;
    p->st = (hipStream_t)stream;
    if (int rc = p->alloc_sets(set_start)) return rc;
    BH_HIP(p->bufs.alloc(p->dep, ndep));
    BH_HIP(p->bufs.alloc(p->cnt, 2 * (size_t)nsets));
    BH_HIP(p->bufs.alloc(p->nlay, (size_t)nsets * (p->maxn + 1)));
    BH_HIP(p->bufs.alloc(p->mfkey, (size_t)p->goff[nsets]));
    BH_HIP(p->bufs.alloc(p->mfrow, (size_t)p->goff[nsets]));
    BH_HIP(hipMemcpyAsync(p->dep, dep, sizeof(double) * ndep, hipMemcpyHostToDevice, p->st));
    if (nifedges) {
        BH_HIP(p->bufs.alloc(p->ifedges, nifedges));
        BH_HIP(p->bufs.alloc(p->ifhist, (size_t)nsets * (nifedges - 1)));
        BH_HIP(hipMemcpyAsync(p->ifedges, ifedges, sizeof(double) * nifedges, hipMemcpyHostToDevice, p->st));
    }
    BH_HIP(hipStreamSynchronize(p->st));
    return BH_OK;
}

// every output but `status` may be NULL
int scan(const char *who, bh_posterior_sets *p, long long *total, double *vmin, double *vmax, double *mean,
         long long *nlayers, long long *ifhist, long long *argmin, int *status)
{
    const int S = p->nsets, nl1 = p->maxn + 1, nih = p->nif > 1 ? p->nif - 1 : 0;
    int rc = p->begin_scan(p->cnt, 2 * (size_t)S);
    if (rc) return rc;
    BH_HIP(hipMemsetAsync(p->nlay, 0, sizeof(u64) * (size_t)S * nl1, p->st));
    if (nih) BH_HIP(hipMemsetAsync(p->ifhist, 0, sizeof(u64) * (size_t)S * nih, p->st));
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
    a.off_if = nl1;
    SetArgs s = set_args(p);
    rc = run<MODE_SCAN>(p, a, s, S, sizeof(u64) * (size_t)(nl1 + nih));
    std::vector<u64> cnt, nl, ih, mk;
    std::vector<long long> mr;
    std::vector<double> sum;
    if (!rc) rc = fetch(cnt, p->cnt, 2 * (size_t)S, p->st);
    if (!rc) rc = fetch(nl, p->nlay, (size_t)S * nl1, p->st);
    if (!rc) rc = fetch(ih, p->ifhist, (size_t)S * nih, p->st);
    if (!rc && p->misfit) rc = fetch(mk, p->mfkey, (size_t)p->goff[S], p->st);
    if (!rc && p->misfit) rc = fetch(mr, p->mfrow, (size_t)p->goff[S], p->st);
    if (!rc) rc = p->reduce_slab(sum);             // synchronises the stream
    if (rc) return rc;
    std::vector<u64> included(S), negative(S);
    for (int z = 0; z < S; z++) {
        included[z] = cnt[2 * (size_t)z];
        negative[z] = cnt[2 * (size_t)z + 1];
    }
    rc = p->end_scan(who, included, negative, sum, total, status, vmin, vmax, mean);
    if (rc) return rc;
    for (int z = 0; z < S; z++) {
        if (nlayers)
            for (int i = 0; i < nl1; i++) nlayers[(size_t)z * nl1 + i] = (long long)nl[(size_t)z * nl1 + i];
        if (ifhist)
            for (int i = 0; i < nih; i++) ifhist[(size_t)z * nih + i] = (long long)ih[(size_t)z * nih + i];
        if (argmin) {
            long long best = -1;
            u64 bk = 0;
            const int G = p->G(z);
            for (int g = 0; p->misfit && g < G; g++) {
                const u64 k = mk[(size_t)p->goff[z] + g];
                const long long r = mr[(size_t)p->goff[z] + g];
                if (r >= 0 && (best < 0 || k < bk || (k == bk && r < best))) { best = r; bk = k; }
            }
            argmin[z] = best;
        }
    }
    return BH_OK;
}

// after a scan
int finish(const char *who, bh_posterior_sets *p, const double *vedges, const int *vedge_off, const int *dbin,
           int ndbins, long long *hist, double *stdev, double *median)
{
    const int D = p->n, S = p->nsets;
    const bool want_hist = vedges != nullptr;
    if (want_hist && (!vedge_off || vedge_off[0] != 0 || !dbin || ndbins < 1 || !hist))
        return bh::fail_who(who, "Vs edges need their offsets (from 0), depth bins and histogram");
    const int tile_fits = want_hist ? tiles_fit(dbin, D, ndbins) : 1;
    if (tile_fits < 0) return bh::fail_who(who, "depth bin out of range");
    std::vector<int> &sflags = p->skip;
    sflags.assign(S, 0);
    std::vector<u64> hoff((size_t)S + 1, 0);
    for (int z = 0; z < S; z++) {
        bool live = p->status[z] == BH_POSTERIOR_SET_OK;
        if (want_hist) {
            const int nve = vedge_off[z + 1] - vedge_off[z];
            if (nve < 0) return bh::fail_who(who, "vedge_off must be ascending");
            if (nve == 0) live = false;          // the caller leaves the set out
            if (live && (nve < 2 || !bh::ascending(vedges + vedge_off[z], nve)))
                return bh::fail_who(who, "a set's Vs edges must be ascending, two at least");
            hoff[z + 1] = hoff[z] + (u64)ndbins * (u64)(nve > 1 ? nve - 1 : 0);
            if (live && (!tile_fits || (size_t)kTile * (nve - 1) * sizeof(u64) > (size_t)kHistLdsBytes))
                sflags[z] |= S_HIST_GLOBAL;
        }
        if (!live) sflags[z] |= S_SKIP;
    }
    bh::CallBufs tmp(p->st);
    PostArgs a = base_args(p);
    a.mean = p->dmean;
    SetArgs s = set_args(p);
    if (int rc = p->upload_skip()) return rc;
    if (want_hist) {
        double *dve = nullptr;
        int *ddb = nullptr, *dvo = nullptr;
        u64 *dho = nullptr;
        const size_t nve_all = (size_t)vedge_off[S], nhist = (size_t)hoff[S];
        BH_HIP(tmp.alloc(dve, nve_all ? nve_all : 1));
        BH_HIP(tmp.alloc(ddb, D));
        BH_HIP(tmp.alloc(dvo, (size_t)S + 1));
        BH_HIP(tmp.alloc(dho, (size_t)S + 1));
        BH_HIP(tmp.alloc(a.hist, nhist ? nhist : 1));
        if (nve_all) BH_HIP(hipMemcpyAsync(dve, vedges, sizeof(double) * nve_all, hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemcpyAsync(ddb, dbin, sizeof(int) * D, hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemcpyAsync(dvo, vedge_off, sizeof(int) * ((size_t)S + 1), hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemcpyAsync(dho, hoff.data(), sizeof(u64) * ((size_t)S + 1), hipMemcpyHostToDevice, p->st));
        if (nhist) BH_HIP(hipMemsetAsync(a.hist, 0, sizeof(u64) * nhist, p->st));
        a.flags |= F_HIST;
        a.vedges = dve;
        a.dbin = ddb;
        a.ndb = ndbins;
        s.vedge_off = dvo;
        s.hist_off = dho;
    }
    if (median) a.flags |= F_RADIX;
    if (stdev) a.flags |= F_SQ;
    const int first_flags = a.flags;
    // LDS: radix digits first, then the histogram tile
    a.off_radix = 0;
    a.off_hist = median ? kTile * 2 * 256 : 0;
    const double nan = std::nan("");
    // sets per chunk: the digit table of the select is what the budget bounds
    const long long fit = (p->chunk_bytes > 0 ? p->chunk_bytes : kDigitBudget) / ((long long)D * 2 * 256 * (long long)sizeof(u64));
    const int chunk = (int)(fit < 1 ? 1 : fit > S ? S : fit);
    for (int first = 0; first < S; first += chunk) {
        const int nc = S - first < chunk ? S - first : chunk;
        s.first = first;
        int tile = 0;                  // the widest LDS histogram tile of the chunk
        for (int z = first; want_hist && z < first + nc; z++)
            if (!(sflags[z] & (S_SKIP | S_HIST_GLOBAL))) {
                const int t = kTile * (vedge_off[z + 1] - vedge_off[z] - 1);
                tile = t > tile ? t : tile;
            }
        // the median: each set's two middle order statistics (0-based), at most two groups a column
        std::vector<uint64_t> ranks;
        if (median) {
            ranks.resize(2 * (size_t)nc * D);
            for (int zl = 0; zl < nc; zl++) {
                const u64 t = (sflags[first + zl] & S_SKIP) ? 0 : p->total[first + zl];
                for (int c = 0; c < D; c++) {
                    ranks[(size_t)zl * D + c] = t ? (t - 1) / 2 : 0;
                    ranks[(size_t)(nc + zl) * D + c] = t / 2;
                }
            }
        }
        bh::CallBufs seltmp(p->st);
        bh::DeviceSelect sel(nc * D, median ? 2 : 0, p->fp64 ? 64 : 32, ranks.data(), bh::RadixSelect::PerColumn());
        if (median) {
            int rc = sel.alloc(seltmp);
            if (rc) return rc;
            a.gbase = sel.dgbase;
            a.ngroups = sel.dngroups;
            a.gpfx = sel.dgpfx;
            a.digits = sel.ddigits;
        }
        a.flags = first_flags;
        size_t lds = sizeof(u64) * (size_t)(a.off_hist + tile);
        for (bool pass1 = true; pass1 || (median && !sel.done()); pass1 = false) {
            int rc = median ? sel.begin_pass(p->st) : BH_OK;
            a.shift = median ? sel.shift : 0;
            if (!rc) rc = run<MODE_FINISH>(p, a, s, nc, lds);
            if (rc) return rc;
            a.flags &= ~(F_SQ | F_HIST | F_HIST_GLOBAL);   // later passes: digits only (they leave the slab alone)
            lds = sizeof(u64) * (size_t)(kTile * 2 * 256);
            if (!median) break;
            rc = sel.end_pass(p->st);
            if (rc) return rc;
        }
        if (median)
            for (int zl = 0; zl < nc; zl++)
                for (int c = 0; c < D; c++)
                    median[(size_t)(first + zl) * D + c] =
                        (sflags[first + zl] & S_SKIP) ? nan : median_of(sel, p->fp64, zl * D + c);
    }
    if (stdev)                         // every chunk's first pass has written its sets' slab rows
        if (int rc = p->read_stdev(stdev)) return rc;
    if (want_hist && hoff[S]) return bh::read_hist(a.hist, (size_t)hoff[S], hist, p->st);
    return BH_OK;
}

template <typename H>
void destroy(H *post)
{
    if (post) {
        (void)hipStreamSynchronize(post->st);
        delete post;
    }
}

}  // namespace

extern "C" {

int bh_posterior_sets_set_chunk_bytes(bh_posterior_sets *p, long long bytes)
{
    if (!p) return bh::fail_arg_("post is NULL");
    p->chunk_bytes = bytes > 0 ? bytes : 0;
    return BH_OK;
}

const char *bh_posterior_sets_status_text(int status)
{
    return bh::set_status_text(status);
}

int bh_posterior_sets_create(const void *rows, int fp64, long long nrows, long long stride, int width,
                             const int *weights, const double *misfits, const long long *set_start, int nsets,
                             const double *dep, int ndep, const double *ifedges, int nifedges, void *stream,
                             bh_posterior_sets **post)
{
    if (!post) return bh::fail_arg_("post is NULL");
    *post = nullptr;
    std::unique_ptr<bh_posterior_sets> p(new (std::nothrow) bh_posterior_sets);
    if (int rc = create("bh_posterior_sets_create", p.get(), rows, fp64, nrows, stride, width, weights, misfits,
                        set_start, nsets, dep, ndep, ifedges, nifedges, stream))
        return rc;
    *post = p.release();
    return BH_OK;
}

void bh_posterior_sets_destroy(bh_posterior_sets *post)
{
    destroy(post);
}

int bh_posterior_sets_scan(bh_posterior_sets *p, long long *total, double *vmin, double *vmax, double *mean,
                           long long *nlayers, long long *ifhist, long long *argmin, int *status)
{
    if (!p) return bh::fail_arg_("post is NULL");
    if (!status) return bh::fail_arg_("bh_posterior_sets_scan: status is NULL");
    return scan("bh_posterior_sets_scan", p, total, vmin, vmax, mean, nlayers, ifhist, argmin, status);
}

int bh_posterior_sets_finish(bh_posterior_sets *p, const double *vedges, const int *vedge_off, const int *dbin,
                             int ndbins, long long *hist, double *stdev, double *median)
{
    if (!p) return bh::fail_arg_("post is NULL");
    if (!p->scanned) return bh::fail_arg_("bh_posterior_sets_finish before bh_posterior_sets_scan");
    return finish("bh_posterior_sets_finish", p, vedges, vedge_off, dbin, ndbins, hist, stdev, median);
}

// ---- all rows as one set: the layouts of the two forms coincide at nsets = 1, so the caller's arrays go through as
// they are; what differs is that a total without statistics is an error here, and that Vs edges are one array --------

int bh_posterior_create(const void *rows, int fp64, long long nrows, long long stride, int width,
                        const int *weights, const double *misfits, const double *dep, int ndep,
                        const double *ifedges, int nifedges, void *stream, bh_posterior **post)
{
    if (!post) return bh::fail_arg_("post is NULL");
    *post = nullptr;
    const long long all[2] = {0, nrows};
    std::unique_ptr<bh_posterior> p(new (std::nothrow) bh_posterior);
    if (int rc = create("bh_posterior_create", p.get(), rows, fp64, nrows, stride, width, weights, misfits, all, 1,
                        dep, ndep, ifedges, nifedges, stream))
        return rc;
    *post = p.release();
    return BH_OK;
}

void bh_posterior_destroy(bh_posterior *post)
{
    destroy(post);
}

int bh_posterior_scan(bh_posterior *p, long long *total, double *vmin, double *vmax, double *mean,
                      long long *nlayers, long long *ifhist, long long *argmin)
{
    if (!p) return bh::fail_arg_("post is NULL");
    long long tot = 0;
    int status = BH_POSTERIOR_SET_OK;
    if (int rc = scan("bh_posterior_scan", p, &tot, vmin, vmax, mean, nlayers, ifhist, argmin, &status)) return rc;
    if (status != BH_POSTERIOR_SET_OK) {           // no statistics: an error, and nothing for a finish to go on
        p->scanned = 0;
        return bh::fail_who("bh_posterior_scan", bh::set_status_text(status));
    }
    if (total) *total = tot;
    return BH_OK;
}

int bh_posterior_finish(bh_posterior *p, const double *vedges, int nvedges, const int *dbin, int ndbins,
                        long long *hist, double *stdev, double *median)
{
    if (!p) return bh::fail_arg_("post is NULL");
    if (!p->scanned) return bh::fail_arg_("bh_posterior_finish before bh_posterior_scan");
    // checked here: to the sets form, a set without edges is a set the caller leaves out
    if (vedges && (nvedges < 2 || !bh::ascending(vedges, nvedges) || !dbin || ndbins < 1 || !hist))
        return bh::fail_arg_("bh_posterior_finish: Vs edges must be ascending, depth bins and histogram given");
    const int vedge_off[2] = {0, nvedges};
    return finish("bh_posterior_finish", p, vedges, vedge_off, dbin, ndbins, hist, stdev, median);
}

}  // extern "C"
