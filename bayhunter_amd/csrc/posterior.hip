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
#include "posterior_core.h"
#include "stats_host.h"

namespace {

using bh::u64;
constexpr int kThreads = 256;
constexpr int kTile = 8;              // depths per blockIdx.y: acc / min / max / prefixes stay in registers
constexpr int kMaxBlocksX = 1024;     // fixed, so that the slab reduction order depends on nrows only
constexpr int kHistLdsBytes = 64 * 1024;

enum { MODE_SCAN = 1, MODE_FINISH = 2 };
enum { F_ROWS = 1, F_SQ = 2, F_HIST = 4, F_RADIX = 8, F_HIST_GLOBAL = 16 };

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
    double *slab;                      // [gridDim.x][D]: Σ w·v (scan) or Σ w·(v-mean)² (finish)
    u64 *cnt;                          // [2]: weight total, rows with a negative weight
    u64 *nlay; int maxn;               // [maxn + 1]
    const double *ifedges; int nif;    // interface-depth edges, histogram [nif - 1]
    u64 *ifhist;
    u64 *mfkey; long long *mfrow;      // [gridDim.x]
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

template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void post_kernel(PostArgs a)
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
    const long long step = (long long)gridDim.x * kThreads;
    for (long long r = (long long)blockIdx.x * kThreads + tid; r < a.nrows; r += step) {
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
            if (tid == 0 && valid[j]) a.slab[(size_t)blockIdx.x * a.D + d0 + j] = s;
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
            a.mfkey[blockIdx.x] = mkey[0];
            a.mfrow[blockIdx.x] = mrow[0];
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
    STATS_HIP(hipGetLastError());
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        bh::fail_arg_("no usable HIP device (libbayhunter_amd has no CPU fallback)");
        return BH_ERR_NO_DEVICE;
    }
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
    long long g = (nrows + kThreads - 1) / kThreads;
    p->G = (int)(g < kMaxBlocksX ? g : kMaxBlocksX);
    int rc = p->alloc_columns();
    if (rc) return rc;
    STATS_HIP(p->bufs.alloc(p->dep, ndep));
    STATS_HIP(p->bufs.alloc(p->cnt, 2));
    STATS_HIP(p->bufs.alloc(p->nlay, p->maxn + 1));
    STATS_HIP(p->bufs.alloc(p->mfkey, p->G));
    STATS_HIP(p->bufs.alloc(p->mfrow, p->G));
    STATS_HIP(hipMemcpyAsync(p->dep, dep, sizeof(double) * ndep, hipMemcpyHostToDevice, p->st));
    if (nifedges) {
        STATS_HIP(p->bufs.alloc(p->ifedges, nifedges));
        STATS_HIP(p->bufs.alloc(p->ifhist, nifedges - 1));
        STATS_HIP(hipMemcpyAsync(p->ifedges, ifedges, sizeof(double) * nifedges, hipMemcpyHostToDevice, p->st));
    }
    STATS_HIP(hipStreamSynchronize(p->st));
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
    STATS_HIP(hipMemsetAsync(p->cnt, 0, sizeof(u64) * 2, p->st));
    STATS_HIP(hipMemsetAsync(p->nlay, 0, sizeof(u64) * (p->maxn + 1), p->st));
    if (p->nif) STATS_HIP(hipMemsetAsync(p->ifhist, 0, sizeof(u64) * (p->nif - 1), p->st));
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
    STATS_HIP(hipMemcpyAsync(cnt, p->cnt, sizeof(cnt), hipMemcpyDeviceToHost, p->st));
    STATS_HIP(hipMemcpyAsync(nl.data(), p->nlay, sizeof(u64) * nl.size(), hipMemcpyDeviceToHost, p->st));
    if (!ih.empty()) STATS_HIP(hipMemcpyAsync(ih.data(), p->ifhist, sizeof(u64) * ih.size(), hipMemcpyDeviceToHost, p->st));
    if (p->misfit) {
        STATS_HIP(hipMemcpyAsync(mk.data(), p->mfkey, sizeof(u64) * p->G, hipMemcpyDeviceToHost, p->st));
        STATS_HIP(hipMemcpyAsync(mr.data(), p->mfrow, sizeof(long long) * p->G, hipMemcpyDeviceToHost, p->st));
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
    bool tile_fits = true;            // a depth tile's bins fit kTile rows of the LDS histogram
    if (want_hist)
        for (int d0 = 0; d0 < D; d0 += kTile) {
            int lo = ndbins, hi = -1;
            for (int d = d0; d < D && d < d0 + kTile; d++) {
                if (dbin[d] < -1 || dbin[d] >= ndbins) return bh::fail_arg_("bh_posterior_finish: depth bin out of range");
                if (dbin[d] >= 0) { lo = dbin[d] < lo ? dbin[d] : lo; hi = dbin[d] > hi ? dbin[d] : hi; }
            }
            if (hi >= 0 && hi - lo >= kTile) tile_fits = false;
        }
    const int nvb = nvedges - 1;
    bh::DevBufs tmp;
    PostArgs a = base_args(p);
    a.mean = p->dmean;
    if (want_hist) {
        double *dve = nullptr;
        int *ddb = nullptr;
        STATS_HIP(tmp.alloc(dve, nvedges));
        STATS_HIP(tmp.alloc(ddb, D));
        STATS_HIP(tmp.alloc(a.hist, (size_t)ndbins * nvb));
        STATS_HIP(hipMemcpyAsync(dve, vedges, sizeof(double) * nvedges, hipMemcpyHostToDevice, p->st));
        STATS_HIP(hipMemcpyAsync(ddb, dbin, sizeof(int) * D, hipMemcpyHostToDevice, p->st));
        STATS_HIP(hipMemsetAsync(a.hist, 0, sizeof(u64) * (size_t)ndbins * nvb, p->st));
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
        for (int d = 0; d < D; d++) {
            double lo, hi;
            if (p->fp64) {
                lo = bh::post_unkey64(sel.key(0, d));
                hi = bh::post_unkey64(sel.key(1, d));
            } else {
                lo = (double)bh::post_unkey32((uint32_t)sel.key(0, d));
                hi = (double)bh::post_unkey32((uint32_t)sel.key(1, d));
            }
            median[d] = (lo + hi) / 2.0;          // np.median: mean of the two middle values
        }
    return BH_OK;
}

}  // extern "C"
