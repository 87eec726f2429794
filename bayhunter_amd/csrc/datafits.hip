// datafits.hip -- column statistics of the modelled data of a block of weighted rows: of many sets of rows at once
// (bh_datafits_sets_*) and of all rows as one set (bh_datafits_*).
//
// The reference looks at the data fit through PlotFromStorage.plot_bestdatafits / plot_rfcorr
// (src/Plotting.py:1054-1150): one plugin call per chain.  Here the forward output of the whole posterior,
// Y[nrows, stride] (ForwardEngine's `out`, first ncols columns), is reduced per column over rows that each
// carry an integer weight, without expanding them.  The shared parts of that weighted column reduction are in
// stats_core.h / stats_host.h (keys, slabs, the scan / finish hand-over, the radix select); what a block does with
// its rows is df_block in datafits_kernel.h:
//
//   mask    before the scan, one wave per row: the row's weight, or 0 when any of its err flags is non-zero
//           or any of its ncols values is NaN (excluded); weighted totals of included / excluded rows,
//           negative weights
//   layout  a block is kCols columns (blockIdx.y) x 32 row lanes; 8 lanes of a wave read 64 contiguous bytes
//           of a row
//   finish  Σ w·(y - mean)² and the histogram over per-column edges in one pass, then the select's passes for
//           up to 16 ranks over the 64-bit keys: a block keeps kGroups groups of its kCols columns in LDS and
//           the groups beyond that are spread over blockIdx.z
//
// A network inverted in one pool (StationPool) is read station by station, and one handle per station would be a few
// thousand rows per launch, i.e. the latency of its launches, copies and synchronisations times the number of
// stations.  So the rows come in contiguous segments, one per set, and a block belongs to one set: it walks the set's
// rows as block x of the G blocks of a set of that many rows, with the set's own outputs.  The slab of a set is added
// in block order, and the mean and the standard deviation leave the host through one expression each: no number of a
// set depends on the set's offset, on its neighbours or on the chunking, and a bh_datafits handle is the sets handle
// with the single set [0, nrows) (the wrappers at the end of the file).
//
//   mask     one launch for all rows; a wave keeps the totals of the set its rows are in and hands them over when
//            its rows move on to another set
//   grid     x: blocks of the largest set (a block beyond its set's G leaves at once), y: column tiles,
//            z: set (scan, finish) or set * slices + group slice (radix passes)
//   slab     the sets' partials one after the other, set z owning G(z) rows from goff[z] (stats_host.h: SetStats):
//            about 1/32 of the matrix in all, so the scan and the finish take every set in one launch
//   chunks   the select's digit table is 256 * 8 B per (rank, column), so the radix passes take the sets in chunks
//            whose table stays under a budget; a set is never split, and nothing a set's blocks compute depends on
//            the chunk
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include "host_common.h"
#include "datafits_kernel.h"

namespace {

using bh::u64;
using namespace bh::fit;
constexpr int kMaxRanks = BH_DATAFITS_MAX_RANKS;

struct SetArgs {
    const long long *start;            // [nsets + 1] rows of set z: start[z] .. start[z + 1]
    const long long *goff;             // [nsets + 1] slab rows before set z: Σ blocks_of over the sets before it
    int first, gz;                     // the launch's first set; group slices per set (1 outside the radix passes)
    const int *skip;                   // [nsets] finish and radix: the set is left out
    int nesets;                        // edge sets per set
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void df_sets_kernel(FitArgs a, SetArgs s)
{
    const int zl = blockIdx.z / s.gz, z = s.first + zl;
    const long long r0 = s.start[z], r1 = s.start[z + 1];
    const int G = blocks_of(r1 - r0), bx = blockIdx.x;
    if (bx >= G) return;
    if (MODE != MODE_SCAN && s.skip[z]) return;
    const size_t col = (size_t)z * a.ncols;
    a.slab += (size_t)s.goff[z] * a.ncols;
    if (MODE == MODE_SCAN) {
        a.kmin += col;
        a.kmax += col;
    }
    if (MODE == MODE_FINISH) {
        a.mean += col;
        if (a.do_hist) {
            a.edges += (size_t)z * s.nesets * a.nedges;
            a.hist += col * (a.nedges - 1);
        }
    }
    if (MODE == MODE_RADIX) {
        a.g0 = (blockIdx.z % s.gz) * kGroups;
        a.gbase += (size_t)zl * a.ncols;
        a.ngroups += (size_t)zl * a.ncols;
    }
    df_block<MODE>(a, r0, r1, bx, G);
}

// one wave per row: its effective weight to wk; cnt[set][3]: included, excluded weight, rows with a negative weight.
// The rows of a wave ascend, so its sets do: lane 0 adds up the set it is in and hands the totals over when it leaves it.
__global__ __launch_bounds__(kThreads) void df_sets_mask_kernel(const double *Y, long long nrows, long long stride,
                                                               int ncols, const int *w, const int *err, int nerr,
                                                               const long long *start, int nsets, int *wk, u64 *cnt)
{
    const int lane = threadIdx.x & 63;
    int z = -1;
    long long end = 0;                                   // the first row past set z, in a register: read once per set
    u64 in = 0, ex = 0, neg = 0;
    const long long waves = (long long)gridDim.x * (kThreads / 64);
    for (long long r = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); r < nrows; r += waves) {
        long long wt;
        const bool bad = mask_row(Y, stride, ncols, w, err, nerr, r, lane, wt);
        if (lane == 0) {
            if (r >= end) {
                if (in) atomicAdd(&cnt[3 * (size_t)z], in);
                if (ex) atomicAdd(&cnt[3 * (size_t)z + 1], ex);
                if (neg) atomicAdd(&cnt[3 * (size_t)z + 2], neg);
                in = ex = neg = 0;
                int lo = z < 0 ? 0 : z + 1, hi = nsets;      // the last set with start <= r (empty sets lie before it)
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (start[mid] <= r) lo = mid;
                    else hi = mid;
                }
                z = lo;
                end = start[z + 1];
            }
            if (wt < 0) neg++;
            else if (bad) ex += (u64)wt;
            else in += (u64)wt;
            wk[r] = (wt > 0 && !bad) ? (int)wt : 0;
        }
    }
    if (lane == 0 && z >= 0) {
        if (in) atomicAdd(&cnt[3 * (size_t)z], in);
        if (ex) atomicAdd(&cnt[3 * (size_t)z + 1], ex);
        if (neg) atomicAdd(&cnt[3 * (size_t)z + 2], neg);
    }
}

}  // namespace

struct bh_datafits_sets : bh::SetStats<blocks_of> {
    int nerr = 0;
    long long chunk_bytes = 0;
    const double *Y = nullptr;
    const int *w = nullptr, *err = nullptr;
    long long nrows = 0, stride = 0;
    // device
    int *wk = nullptr;                 // [nrows]
    u64 *cnt = nullptr;                // [nsets][3]
};

struct bh_datafits : bh_datafits_sets {};          // all rows as the one set of the handle

namespace {

FitArgs base_args(const bh_datafits_sets *p)
{
    FitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.Y = p->Y;
    a.nrows = p->nrows;
    a.stride = p->stride;
    a.ncols = p->n;
    a.wk = p->wk;
    a.slab = p->slab;
    return a;
}

SetArgs set_args(const bh_datafits_sets *p)
{
    SetArgs s;
    std::memset(&s, 0, sizeof(s));
    s.start = p->dstart;
    s.goff = p->dgoff;
    s.gz = 1;
    s.skip = p->dskip;
    return s;
}

// sets [s.first, s.first + nc), s.gz group slices each
template <int MODE>
int launch(bh_datafits_sets *p, const FitArgs &a, const SetArgs &s, int nc, size_t lds)
{
    dim3 grid((unsigned)p->chunk_blocks(s.first, nc), (unsigned)((p->n + kCols - 1) / kCols), (unsigned)(nc * s.gz));
    hipLaunchKernelGGL((df_sets_kernel<MODE>), grid, dim3(kThreads), lds, p->st, a, s);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// ---- the three steps of a handle; `who` is the entry point that reports what they refuse ------------------------

// the arguments, then the fresh handle `p` (NULL: there was no memory for it) with its device buffers
int create(const char *who, bh_datafits_sets *p, const double *Y, long long nrows, long long stride, int ncols,
           const int *weights, const int *err, int nerr, const long long *set_start, int nsets, void *stream)
{
    if (!Y || nrows < 1) return bh::fail_who(who, "no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_who(who, "more than 2^32 rows (the weight total could overflow)");
    if (ncols < 1) return bh::fail_who(who, "ncols < 1");
    if (stride < ncols) return bh::fail_who(who, "stride < ncols");
    if (err && nerr < 1) return bh::fail_who(who, "err flags given with nerr < 1");
    if (nsets < 1 || nsets > kMaxGridZ) return bh::fail_who(who, "1 to 65535 sets");
    if (int rc = bh::check_set_start(who, set_start, nsets, nrows)) return rc;
    if ((long long)nsets * ncols > 0x3fffffff) return bh::fail_who(who, "more than 2^30 (set, column) pairs");
    if (int rc = bh::require_device()) return rc;
    if (!p) return bh::fail_arg_("out of memory");
    p->Y = Y;
    p->nrows = nrows;
    p->stride = stride;
    p->n = ncols;
    p->w = weights;
    p->err = err;
    p->nerr = err ? nerr : 0;
    p->nsets = nsets;
    p->st = (hipStream_t)stream;
    if (int rc = p->alloc_sets(set_start)) return rc;
    BH_HIP(p->bufs.alloc(p->wk, (size_t)nrows));
    BH_HIP(p->bufs.alloc(p->cnt, 3 * (size_t)nsets));
    BH_HIP(hipStreamSynchronize(p->st));
    return BH_OK;
}

// every output but `status` may be NULL
int scan(const char *who, bh_datafits_sets *p, long long *total, long long *excluded, double *vmin, double *vmax,
         double *mean, int *status)
{
    const int N = p->n, S = p->nsets;
    int rc = p->begin_scan(p->cnt, 3 * (size_t)S);
    if (rc) return rc;
    {
        const long long blocks = (p->nrows + kThreads / 64 - 1) / (kThreads / 64);
        hipLaunchKernelGGL(df_sets_mask_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kThreads), 0, p->st,
                           p->Y, p->nrows, p->stride, N, p->w, p->err, p->nerr, (const long long *)p->dstart, S, p->wk,
                           p->cnt);
        BH_HIP(hipGetLastError());
    }
    FitArgs a = base_args(p);
    a.kmin = p->kmin;
    a.kmax = p->kmax;
    SetArgs s = set_args(p);
    rc = launch<MODE_SCAN>(p, a, s, S, 0);
    if (rc) return rc;
    std::vector<u64> cnt(3 * (size_t)S);
    BH_HIP(hipMemcpyAsync(cnt.data(), p->cnt, sizeof(u64) * cnt.size(), hipMemcpyDeviceToHost, p->st));
    std::vector<double> sum;
    rc = p->reduce_slab(sum);                      // synchronises the stream
    if (rc) return rc;
    std::vector<u64> included(S), negative(S);
    for (int z = 0; z < S; z++) {
        included[z] = cnt[3 * (size_t)z];
        negative[z] = cnt[3 * (size_t)z + 2];
    }
    rc = p->end_scan(who, included, negative, sum, total, status, vmin, vmax, mean);
    if (rc) return rc;
    for (int z = 0; excluded && z < S; z++) excluded[z] = (long long)cnt[3 * (size_t)z + 1];
    return BH_OK;
}

// what a finish checks of its arguments without a handle or a device: the ranks, the edges
int check_ranks(const char *who, const long long *ranks, int nranks, const double *order_stats)
{
    if (nranks < 0 || nranks > kMaxRanks) return bh::fail_who(who, "0 to 16 ranks");
    if (nranks && (!ranks || !order_stats)) return bh::fail_who(who, "ranks and order_stats");
    return BH_OK;
}

int check_edges(const char *who, const double *edges, int nedges, int nesets, const int *eset, const long long *hist)
{
    if (edges && (nedges < 2 || nesets < 1 || !eset || !hist))
        return bh::fail_who(who, "edges need nedges >= 2, nsets >= 1, eset and hist");
    return BH_OK;
}

// after a scan and the two checks above: what the scan decides, then the launches
int finish(const char *who, bh_datafits_sets *p, const long long *ranks, int nranks, double *order_stats,
           const double *edges, int nedges, int nesets, const int *eset, long long *hist, double *stdev)
{
    const bool want_hist = edges != nullptr;
    const int N = p->n, S = p->nsets;
    std::vector<int> &skip = p->skip;
    for (int z = 0; z < S; z++) {
        skip[z] = p->status[z] != BH_DATAFITS_SET_OK ? bh::SET_SKIP : 0;
        if (skip[z]) continue;
        for (int i = 0; i < nranks; i++) {
            const long long r = ranks[(size_t)z * nranks + i];
            if (r < 0) return bh::fail_who(who, "negative rank");
            if ((u64)r >= p->total[z]) return bh::fail_who(who, "rank >= the weight total");
        }
        for (int e = 0; want_hist && e < nesets; e++)
            if (!bh::ascending(edges + ((size_t)z * nesets + e) * nedges, nedges))
                return bh::fail_who(who, "edges must be ascending");
    }
    if (want_hist)
        for (int c = 0; c < N; c++)
            if (eset[c] < 0 || eset[c] >= nesets) return bh::fail_who(who, "edge set out of range");

    bh::CallBufs tmp(p->st);
    const int nb = nedges - 1;
    const size_t cols = (size_t)S * N;
    const double nan = std::nan("");
    if (int rc = p->upload_skip()) return rc;
    if (stdev || want_hist) {
        FitArgs a = base_args(p);
        a.mean = p->dmean;
        SetArgs s = set_args(p);
        size_t lds = 0;
        if (want_hist) {
            double *ded = nullptr;
            int *dset = nullptr;
            const size_t ne = (size_t)S * nesets * nedges;
            BH_HIP(tmp.alloc(ded, ne));
            BH_HIP(tmp.alloc(dset, N));
            BH_HIP(tmp.alloc(a.hist, cols * nb));
            BH_HIP(hipMemcpyAsync(ded, edges, sizeof(double) * ne, hipMemcpyHostToDevice, p->st));
            BH_HIP(hipMemcpyAsync(dset, eset, sizeof(int) * N, hipMemcpyHostToDevice, p->st));
            BH_HIP(hipMemsetAsync(a.hist, 0, sizeof(u64) * cols * nb, p->st));
            a.edges = ded;
            a.nedges = nedges;
            a.eset = dset;
            a.do_hist = 1;
            a.hist_lds = (size_t)kCols * nb * sizeof(u64) <= (size_t)kHistLdsBytes;
            lds = a.hist_lds ? (size_t)kCols * nb * sizeof(u64) : 0;
            s.nesets = nesets;
        }
        int rc = launch<MODE_FINISH>(p, a, s, S, lds);
        if (!rc && stdev) rc = p->read_stdev(stdev);                 // synchronises the stream
        if (!rc && want_hist) rc = bh::read_hist(a.hist, cols * nb, hist, p->st);
        if (rc) return rc;
    }
    if (!nranks) return BH_OK;

    const int gz_max = (nranks + kGroups - 1) / kGroups;
    const int chunk = sets_per_chunk(S, N, nranks, gz_max, p->chunk_bytes);
    FitArgs r = base_args(p);
    SetArgs s = set_args(p);
    std::vector<uint64_t> rk;
    for (int first = 0; first < S; first += chunk) {
        const int nc = S - first < chunk ? S - first : chunk;
        // every set its own ranks, because the weight totals differ: [nranks][nc * N]
        rk.assign((size_t)nranks * nc * N, 0);
        for (int i = 0; i < nranks; i++)
            for (int zl = 0; zl < nc; zl++) {
                const uint64_t v = skip[first + zl] ? 0 : (uint64_t)ranks[(size_t)(first + zl) * nranks + i];
                for (int c = 0; c < N; c++) rk[((size_t)i * nc + zl) * N + c] = v;
            }
        bh::CallBufs seltmp(p->st);
        bh::DeviceSelect sel(nc * N, nranks, 64, rk.data(), bh::RadixSelect::PerColumn());
        int rc = sel.alloc(seltmp);
        if (rc) return rc;
        r.gbase = sel.dgbase;
        r.ngroups = sel.dngroups;
        r.gpfx = sel.dgpfx;
        r.digits = sel.ddigits;
        s.first = first;
        while (!sel.done()) {
            rc = sel.begin_pass(p->st);
            r.shift = sel.shift;
            s.gz = (sel.maxgroups + kGroups - 1) / kGroups;
            if (!rc) rc = launch<MODE_RADIX>(p, r, s, nc, sizeof(u64) * kCols * kGroups * 256);
            if (!rc) rc = sel.end_pass(p->st);
            if (rc) return rc;
        }
        for (int zl = 0; zl < nc; zl++)
            for (int i = 0; i < nranks; i++)
                for (int c = 0; c < N; c++)
                    order_stats[((size_t)(first + zl) * nranks + i) * N + c] =
                        skip[first + zl] ? nan : bh::post_unkey64(sel.key(i, zl * N + c));
    }
    return BH_OK;
}

template <typename H>
void destroy(H *fits)
{
    if (fits) {
        (void)hipStreamSynchronize(fits->st);
        delete fits;
    }
}

}  // namespace

extern "C" {

const char *bh_datafits_sets_status_text(int status)
{
    return bh::set_status_text(status);
}

int bh_datafits_sets_set_chunk_bytes(bh_datafits_sets *p, long long bytes)
{
    if (!p) return bh::fail_arg_("fits is NULL");
    p->chunk_bytes = bytes > 0 ? bytes : 0;
    return BH_OK;
}

int bh_datafits_sets_create(const double *Y, long long nrows, long long stride, int ncols, const int *weights,
                            const int *err, int nerr, const long long *set_start, int nsets, void *stream,
                            bh_datafits_sets **fits)
{
    if (!fits) return bh::fail_arg_("fits is NULL");
    *fits = nullptr;
    std::unique_ptr<bh_datafits_sets> p(new (std::nothrow) bh_datafits_sets);
    if (int rc = create("bh_datafits_sets_create", p.get(), Y, nrows, stride, ncols, weights, err, nerr, set_start,
                        nsets, stream))
        return rc;
    *fits = p.release();
    return BH_OK;
}

void bh_datafits_sets_destroy(bh_datafits_sets *fits)
{
    destroy(fits);
}

int bh_datafits_sets_scan(bh_datafits_sets *p, long long *total, long long *excluded, double *vmin, double *vmax,
                          double *mean, int *status)
{
    if (!p) return bh::fail_arg_("fits is NULL");
    if (!status) return bh::fail_arg_("bh_datafits_sets_scan: status is NULL");
    return scan("bh_datafits_sets_scan", p, total, excluded, vmin, vmax, mean, status);
}

int bh_datafits_sets_finish(bh_datafits_sets *p, const long long *ranks, int nranks, double *order_stats,
                            const double *edges, int nedges, int nesets, const int *eset, long long *hist,
                            double *stdev)
{
    // the arguments first: what needs no handle, then what the scan decides; nothing is launched before
    const char *who = "bh_datafits_sets_finish";
    if (int rc = check_ranks(who, ranks, nranks, order_stats)) return rc;
    if (int rc = check_edges(who, edges, nedges, nesets, eset, hist)) return rc;
    if (!p) return bh::fail_arg_("fits is NULL");
    if (!p->scanned) return bh::fail_arg_("bh_datafits_sets_finish before a successful bh_datafits_sets_scan");
    return finish(who, p, ranks, nranks, order_stats, edges, nedges, nesets, eset, hist, stdev);
}

// ---- all rows as one set: the layouts of the two forms coincide at nsets = 1, so the caller's arrays go through as
// they are; what differs is that a total without statistics is an error here ------------------------------------------

int bh_datafits_create(const double *Y, long long nrows, long long stride, int ncols, const int *weights,
                       const int *err, int nerr, void *stream, bh_datafits **fits)
{
    if (!fits) return bh::fail_arg_("fits is NULL");
    *fits = nullptr;
    const long long all[2] = {0, nrows};
    std::unique_ptr<bh_datafits> p(new (std::nothrow) bh_datafits);
    if (int rc = create("bh_datafits_create", p.get(), Y, nrows, stride, ncols, weights, err, nerr, all, 1, stream))
        return rc;
    *fits = p.release();
    return BH_OK;
}

void bh_datafits_destroy(bh_datafits *fits)
{
    destroy(fits);
}

int bh_datafits_scan(bh_datafits *p, long long *total, long long *excluded, double *vmin, double *vmax,
                     double *mean)
{
    if (!p) return bh::fail_arg_("fits is NULL");
    long long tot = 0, exc = 0;
    int status = BH_DATAFITS_SET_OK;
    if (int rc = scan("bh_datafits_scan", p, &tot, &exc, vmin, vmax, mean, &status)) return rc;
    if (excluded) *excluded = exc;                 // reported for an empty selection too: all of it may be excluded
    if (total) *total = tot;
    if (status != BH_DATAFITS_SET_OK) {            // no statistics: an error, and nothing for a finish to go on
        p->scanned = 0;
        return bh::fail_who("bh_datafits_scan", bh::set_status_text(status));
    }
    return BH_OK;
}

int bh_datafits_finish(bh_datafits *p, const long long *ranks, int nranks, double *order_stats,
                       const double *edges, int nedges, int nsets, const int *eset, long long *hist, double *stdev)
{
    // the arguments first: checked without a handle or a device
    const char *who = "bh_datafits_finish";
    if (int rc = check_ranks(who, ranks, nranks, order_stats)) return rc;
    for (int i = 0; i < nranks; i++)
        if (ranks[i] < 0) return bh::fail_who(who, "negative rank");
    if (int rc = check_edges(who, edges, nedges, nsets, eset, hist)) return rc;
    for (int s = 0; edges && s < nsets; s++)
        if (!bh::ascending(edges + (size_t)s * nedges, nedges)) return bh::fail_who(who, "edges must be ascending");
    if (!p) return bh::fail_arg_("fits is NULL");
    if (!p->scanned) return bh::fail_arg_("bh_datafits_finish before a successful bh_datafits_scan");
    return finish(who, p, ranks, nranks, order_stats, edges, nedges, nsets, eset, hist, stdev);
}

}  // extern "C"
