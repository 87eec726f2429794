// datafits.hip -- column statistics of the modelled data of a block of weighted rows (bh_datafits_*).
//
// The reference looks at the data fit through PlotFromStorage.plot_bestdatafits / plot_rfcorr
// (src/Plotting.py:1054-1150): one plugin call per chain.  Here the forward output of the whole posterior,
// Y[nrows, stride] (ForwardEngine's `out`, first ncols columns), is reduced per column over rows that each
// carry an integer weight, without expanding them.  The shared parts of that weighted column reduction are in
// stats_core.h / stats_host.h (keys, slabs, the scan / finish hand-over, the radix select); what a block does with
// its rows is df_block in datafits_kernel.h, which datafits_sets.hip runs too (one set per block); this file has
// the handle of one set:
//
//   mask    before the scan, one wave per row: the row's weight, or 0 when any of its err flags is non-zero
//           or any of its ncols values is NaN (excluded); weighted totals of included / excluded rows,
//           negative weights
//   layout  a block is kCols columns (blockIdx.y) x 32 row lanes; 8 lanes of a wave read 64 contiguous bytes
//           of a row
//   finish  Σ w·(y - mean)² and the histogram over per-column edges in one pass, then the select's passes for
//           up to 16 ranks over the 64-bit keys: a block keeps kGroups groups of its kCols columns in LDS and
//           the groups beyond that are spread over blockIdx.z
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

// one wave per row: effective weights and the totals of included / excluded weight
__global__ __launch_bounds__(kThreads) void df_mask_kernel(const double *Y, long long nrows, long long stride,
                                                          int ncols, const int *w, const int *err, int nerr,
                                                          int *wk, u64 *cnt)
{
    __shared__ u64 s_in, s_ex, s_neg;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) { s_in = 0; s_ex = 0; s_neg = 0; }
    __syncthreads();
    u64 in = 0, ex = 0, neg = 0;
    const long long waves = (long long)gridDim.x * (kThreads / 64);
    for (long long r = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); r < nrows; r += waves) {
        long long wt;
        const bool bad = mask_row(Y, stride, ncols, w, err, nerr, r, lane, wt);
        if (lane == 0) {
            if (wt < 0) neg++;
            else if (bad) ex += (u64)wt;
            else in += (u64)wt;
            wk[r] = (wt > 0 && !bad) ? (int)wt : 0;
        }
    }
    if (lane == 0) {
        if (in) atomicAdd(&s_in, in);
        if (ex) atomicAdd(&s_ex, ex);
        if (neg) atomicAdd(&s_neg, neg);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_in) atomicAdd(&cnt[0], s_in);
        if (s_ex) atomicAdd(&cnt[1], s_ex);
        if (s_neg) atomicAdd(&cnt[2], s_neg);
    }
}

// all rows are one set: block blockIdx.x of gridDim.x, group slice blockIdx.z (datafits_kernel.h)
template <int MODE>
__global__ __launch_bounds__(kThreads) void df_kernel(FitArgs a)
{
    a.g0 = blockIdx.z * kGroups;
    df_block<MODE>(a, 0, a.nrows, blockIdx.x, gridDim.x);
}

}  // namespace

struct bh_datafits : bh::ColumnStats {           // n: the columns
    int nerr = 0;
    const double *Y = nullptr;
    const int *w = nullptr, *err = nullptr;
    long long nrows = 0, stride = 0;
    // device
    int *wk = nullptr;
    u64 *cnt = nullptr;
};

namespace {

FitArgs base_args(const bh_datafits *p)
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

template <int MODE>
int launch(bh_datafits *p, const FitArgs &a, int gz, size_t lds)
{
    dim3 grid((unsigned)p->G, (unsigned)((p->n + kCols - 1) / kCols), (unsigned)gz);
    hipLaunchKernelGGL((df_kernel<MODE>), grid, dim3(kThreads), lds, p->st, a);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

}  // namespace

extern "C" {

int bh_datafits_create(const double *Y, long long nrows, long long stride, int ncols, const int *weights,
                       const int *err, int nerr, void *stream, bh_datafits **fits)
{
    if (!fits) return bh::fail_arg_("fits is NULL");
    *fits = nullptr;
    if (!Y || nrows < 1) return bh::fail_arg_("bh_datafits_create: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_datafits_create: more than 2^32 rows (the weight total could overflow)");
    if (ncols < 1) return bh::fail_arg_("bh_datafits_create: ncols < 1");
    if (stride < ncols) return bh::fail_arg_("bh_datafits_create: stride < ncols");
    if (err && nerr < 1) return bh::fail_arg_("bh_datafits_create: err flags given with nerr < 1");
    if (int rc = bh::require_device()) return rc;
    std::unique_ptr<bh_datafits> p(new (std::nothrow) bh_datafits);
    if (!p) return bh::fail_arg_("out of memory");
    p->Y = Y;
    p->nrows = nrows;
    p->stride = stride;
    p->n = ncols;
    p->w = weights;
    p->err = err;
    p->nerr = err ? nerr : 0;
    p->st = (hipStream_t)stream;
    p->G = blocks_of(nrows);
    int rc = p->alloc_columns();
    if (rc) return rc;
    BH_HIP(p->bufs.alloc(p->wk, (size_t)nrows));
    BH_HIP(p->bufs.alloc(p->cnt, 3));
    *fits = p.release();
    return BH_OK;
}

void bh_datafits_destroy(bh_datafits *fits)
{
    if (fits) {
        (void)hipStreamSynchronize(fits->st);
        delete fits;
    }
}

int bh_datafits_scan(bh_datafits *p, long long *total, long long *excluded, double *vmin, double *vmax,
                     double *mean)
{
    if (!p) return bh::fail_arg_("fits is NULL");
    int rc = p->begin_scan();
    if (rc) return rc;
    BH_HIP(hipMemsetAsync(p->cnt, 0, sizeof(u64) * 3, p->st));
    {
        long long waves = p->nrows;
        long long blocks = (waves + kThreads / 64 - 1) / (kThreads / 64);
        hipLaunchKernelGGL(df_mask_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kThreads), 0, p->st,
                           p->Y, p->nrows, p->stride, p->n, p->w, p->err, p->nerr, p->wk, p->cnt);
        BH_HIP(hipGetLastError());
    }
    FitArgs a = base_args(p);
    a.kmin = p->kmin;
    a.kmax = p->kmax;
    rc = launch<MODE_SCAN>(p, a, 1, 0);
    if (rc) return rc;
    u64 cnt[3];                                    // included, excluded weight; rows with a negative weight
    BH_HIP(hipMemcpyAsync(cnt, p->cnt, sizeof(cnt), hipMemcpyDeviceToHost, p->st));
    std::vector<double> sum;
    rc = p->reduce_slab(sum);                      // synchronises the stream
    if (rc) return rc;
    if (!cnt[2]) {                                 // reported for an empty selection too: all of it may be excluded
        if (excluded) *excluded = (long long)cnt[1];
        if (total) *total = (long long)cnt[0];
    }
    return p->end_scan("bh_datafits_scan", cnt[0], cnt[2], sum, vmin, vmax, mean);
}

int bh_datafits_finish(bh_datafits *p, const long long *ranks, int nranks, double *order_stats,
                       const double *edges, int nedges, int nsets, const int *eset, long long *hist, double *stdev)
{
    // the arguments first: checked without a handle or a device
    if (nranks < 0 || nranks > kMaxRanks) return bh::fail_arg_("bh_datafits_finish: 0 to 16 ranks");
    if (nranks && (!ranks || !order_stats)) return bh::fail_arg_("bh_datafits_finish: ranks and order_stats");
    for (int i = 0; i < nranks; i++)
        if (ranks[i] < 0) return bh::fail_arg_("bh_datafits_finish: negative rank");
    const bool want_hist = edges != nullptr;
    if (want_hist) {
        if (nedges < 2 || nsets < 1 || !eset || !hist)
            return bh::fail_arg_("bh_datafits_finish: edges need nedges >= 2, nsets >= 1, eset and hist");
        for (int s = 0; s < nsets; s++)
            if (!bh::ascending(edges + (size_t)s * nedges, nedges)) return bh::fail_arg_("bh_datafits_finish: edges must be ascending");
    }
    if (!p) return bh::fail_arg_("fits is NULL");
    if (!p->scanned) return bh::fail_arg_("bh_datafits_finish before a successful bh_datafits_scan");
    const int N = p->n;
    for (int i = 0; i < nranks; i++)
        if ((u64)ranks[i] >= p->total) return bh::fail_arg_("bh_datafits_finish: rank >= the weight total");
    if (want_hist)
        for (int c = 0; c < N; c++)
            if (eset[c] < 0 || eset[c] >= nsets) return bh::fail_arg_("bh_datafits_finish: edge set out of range");

    bh::DevBufs tmp;
    const int nb = nedges - 1;
    if (stdev || want_hist) {
        FitArgs a = base_args(p);
        a.mean = p->dmean;
        size_t lds = 0;
        if (want_hist) {
            double *ded = nullptr;
            int *dset = nullptr;
            BH_HIP(tmp.alloc(ded, (size_t)nsets * nedges));
            BH_HIP(tmp.alloc(dset, N));
            BH_HIP(tmp.alloc(a.hist, (size_t)N * nb));
            BH_HIP(hipMemcpyAsync(ded, edges, sizeof(double) * (size_t)nsets * nedges, hipMemcpyHostToDevice, p->st));
            BH_HIP(hipMemcpyAsync(dset, eset, sizeof(int) * N, hipMemcpyHostToDevice, p->st));
            BH_HIP(hipMemsetAsync(a.hist, 0, sizeof(u64) * (size_t)N * nb, p->st));
            a.edges = ded;
            a.nedges = nedges;
            a.eset = dset;
            a.do_hist = 1;
            a.hist_lds = (size_t)kCols * nb * sizeof(u64) <= (size_t)kHistLdsBytes;
            lds = a.hist_lds ? (size_t)kCols * nb * sizeof(u64) : 0;
        }
        int rc = launch<MODE_FINISH>(p, a, 1, lds);
        if (!rc && stdev) rc = p->read_stdev(stdev);                // either one synchronises the stream
        if (!rc && want_hist) rc = bh::read_hist(a.hist, (size_t)N * nb, hist, p->st);
        if (rc) return rc;
    }
    if (!nranks) return BH_OK;

    uint64_t rk[kMaxRanks];
    for (int i = 0; i < nranks; i++) rk[i] = (uint64_t)ranks[i];
    bh::DeviceSelect sel(N, nranks, 64, rk);
    int rc = sel.alloc(tmp);
    if (rc) return rc;
    FitArgs r = base_args(p);
    r.gbase = sel.dgbase;
    r.ngroups = sel.dngroups;
    r.gpfx = sel.dgpfx;
    r.digits = sel.ddigits;
    while (!sel.done()) {
        rc = sel.begin_pass(p->st);
        r.shift = sel.shift;
        if (!rc) rc = launch<MODE_RADIX>(p, r, (sel.maxgroups + kGroups - 1) / kGroups, sizeof(u64) * kCols * kGroups * 256);
        if (!rc) rc = sel.end_pass(p->st);
        if (rc) return rc;
    }
    for (int i = 0; i < nranks; i++)
        for (int c = 0; c < N; c++) order_stats[(size_t)i * N + c] = bh::post_unkey64(sel.key(i, c));
    return BH_OK;
}

}  // extern "C"
