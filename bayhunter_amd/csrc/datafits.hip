// datafits.hip -- column statistics of the modelled data of a block of weighted rows (bh_datafits_*).
//
// The reference looks at the data fit through PlotFromStorage.plot_bestdatafits / plot_rfcorr
// (src/Plotting.py:1054-1150): one plugin call per chain.  Here the forward output of the whole posterior,
// Y[nrows, stride] (ForwardEngine's `out`, first ncols columns), is reduced per column over rows that each
// carry an integer weight, without expanding them.
//
//   mask    one wave per row: the row's weight, or 0 when any of its err flags is non-zero or any of its
//           ncols values is NaN (excluded); weighted totals of included / excluded rows, negative weights
//   scan    per column: min / max (order-preserving integer keys, integer atomics), Σ w·y (per-block slab
//           reduced in a fixed order)
//   finish  Σ w·(y - mean)² (slab), the histogram over per-column edges, and up to 16 exact weighted order
//           statistics: an 8-bit radix select over the 64-bit keys, one pass per digit.  Ranks whose prefixes
//           still agree share one digit histogram ("group"); a block keeps kGroups groups of its kCols columns
//           in LDS and the groups beyond that are spread over blockIdx.z
//
// Layout: a block is kCols columns (blockIdx.y) x 32 row lanes; 8 lanes of a wave read 64 contiguous bytes
// of a row.  The grid width depends on nrows only, so the slab order -- and every result -- is the same
// from one call to the next.  No floating-point atomics.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>
#include "../../include/bayhunter_amd.h"
#include "posterior_core.h"

namespace bh { int fail_arg_(const char *what); int fail_hip_(int e, const char *what); }

namespace {

#define DF_HIP(call)                                                         \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return bh::fail_hip_((int)e_, #call);          \
    } while (0)

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kCols = 8;                        // columns per blockIdx.y
constexpr int kRowLanes = kThreads / kCols;     // rows a block reads at once
constexpr int kGroups = 4;                      // digit histograms per column and block (LDS 8 * 4 * 256 * 8 B = 64 KiB)
constexpr int kMaxBlocksX = 1024;               // fixed, so that the slab order depends on nrows only
constexpr int kHistLdsBytes = 64 * 1024;
constexpr int kMaxRanks = BH_DATAFITS_MAX_RANKS;

enum { MODE_SCAN = 1, MODE_FINISH = 2, MODE_RADIX = 3 };

struct FitArgs {
    const double *Y;
    long long nrows, stride;
    int ncols;
    const int *wk;                     // [nrows] effective weight (0: skip)
    double *slab;                      // [gridDim.x][ncols]
    // scan
    u64 *kmin, *kmax;                  // [ncols]
    // finish
    const double *mean;                // [ncols]
    const double *edges; int nedges;   // [nsets][nedges]
    const int *eset;                   // [ncols]
    u64 *hist;                         // [ncols][nedges - 1]
    int do_hist, hist_lds;
    // radix
    int shift;                         // digit (key >> shift) & 255
    const int *gbase, *ngroups;        // [ncols]: first slot of the column's groups, their number
    const u64 *gpfx;                   // [slots] prefix (key >> (shift + 8)) of each group
    u64 *digits;                       // [slots][256]
};

// Σ over the 32 row lanes of each column, in lane order: thread (rl, cl) -> column cl
__device__ __forceinline__ double lanes_sum(double v, double *red, int tid)
{
    red[tid] = v;
    __syncthreads();
    double s = 0.0;
    if (tid < kCols)
        for (int l = 0; l < kRowLanes; l++) s = s + red[l * kCols + tid];
    __syncthreads();
    return s;
}

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
        const long long wt = w ? (long long)w[r] : 1;
        bool bad = false;
        const double *row = Y + r * stride;
        for (int c = lane; c < ncols; c += 64) bad |= !(row[c] == row[c]);
        if (err)
            for (int f = lane; f < nerr; f += 64) bad |= err[r * nerr + f] != 0;
        bad = __any(bad);
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

template <int MODE>
__global__ __launch_bounds__(kThreads) void df_kernel(FitArgs a)
{
    extern __shared__ u64 lds[];
    __shared__ double red[kThreads];
    __shared__ u64 smin[kCols], smax[kCols];
    const int tid = threadIdx.x;
    const int cl = tid % kCols, rl = tid / kCols;
    const int c = blockIdx.y * kCols + cl;
    const bool valid = c < a.ncols;
    const int cc = valid ? c : a.ncols - 1;

    // radix: the groups [g0, g0 + kGroups) of this column that this block counts
    const int g0 = blockIdx.z * kGroups;
    int ng = 0, slot0 = 0;
    u64 pf[kGroups];
#pragma unroll
    for (int j = 0; j < kGroups; j++) pf[j] = 0;
    if (MODE == MODE_RADIX) {
        if (valid) {
            ng = a.ngroups[c] - g0;
            ng = ng < 0 ? 0 : (ng > kGroups ? kGroups : ng);
            slot0 = a.gbase[c] + g0;
#pragma unroll
            for (int j = 0; j < kGroups; j++) pf[j] = j < ng ? a.gpfx[slot0 + j] : 0;
        }
        // nothing to count in this slice for any column of the tile: the whole block leaves
        int any = 0;
        for (int j = 0; j < kCols; j++) {
            const int cj = blockIdx.y * kCols + j;
            any |= cj < a.ncols && a.ngroups[cj] > g0;
        }
        if (!any) return;
    }
    const bool whole = MODE == MODE_RADIX && a.shift + 8 >= 64;
    const int nb = a.nedges - 1;
    const double *ed = MODE == MODE_FINISH && a.do_hist ? a.edges + (size_t)a.eset[cc] * a.nedges : nullptr;
    const double mu = MODE == MODE_FINISH ? a.mean[cc] : 0.0;

    int nlds = 0;
    if (MODE == MODE_RADIX) nlds = kCols * kGroups * 256;
    if (MODE == MODE_FINISH && a.do_hist && a.hist_lds) nlds = kCols * nb;
    for (int i = tid; i < nlds; i += kThreads) lds[i] = 0;
    if (tid < kCols) { smin[tid] = ~0ull; smax[tid] = 0ull; }
    __syncthreads();

    double acc = 0.0;
    u64 mn = ~0ull, mx = 0ull;
    const long long step = (long long)gridDim.x * kRowLanes;
    for (long long r = (long long)blockIdx.x * kRowLanes + rl; r < a.nrows; r += step) {
        const int w = a.wk[r];
        if (w == 0 || !valid) continue;
        const double y = a.Y[r * a.stride + c];
        if (MODE == MODE_SCAN) {
            acc = acc + (double)w * y;
            const u64 k = bh::post_key64(y);
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        } else if (MODE == MODE_FINISH) {
            const double e = y - mu;
            acc = acc + (double)w * (e * e);
            const int b = a.do_hist ? bh::post_bin(ed, a.nedges, y) : -1;
            if (b >= 0) {
                if (a.hist_lds) atomicAdd(&lds[cl * nb + b], (u64)w);
                else atomicAdd(&a.hist[(size_t)c * nb + b], (u64)w);
            }
        } else {
            const u64 k = bh::post_key64(y);
            const u64 hi = whole ? 0ull : (k >> (a.shift + 8));
            const int dig = (int)((k >> a.shift) & 255u);
#pragma unroll
            for (int j = 0; j < kGroups; j++)
                if (j < ng && hi == pf[j]) atomicAdd(&lds[(cl * kGroups + j) * 256 + dig], (u64)w);
        }
    }

    if (MODE != MODE_RADIX) {
        const double s = lanes_sum(acc, red, tid);
        if (tid < kCols && blockIdx.y * kCols + tid < a.ncols)
            a.slab[(size_t)blockIdx.x * a.ncols + blockIdx.y * kCols + tid] = s;
    }
    if (MODE == MODE_SCAN) {
        if (mn != ~0ull) atomicMin(&smin[cl], mn);
        if (mx != 0ull) atomicMax(&smax[cl], mx);
        __syncthreads();
        if (tid < kCols && blockIdx.y * kCols + tid < a.ncols) {
            if (smin[tid] != ~0ull) atomicMin(&a.kmin[blockIdx.y * kCols + tid], smin[tid]);
            if (smax[tid] != 0ull) atomicMax(&a.kmax[blockIdx.y * kCols + tid], smax[tid]);
        }
    }
    if (MODE == MODE_FINISH && a.do_hist && a.hist_lds) {
        __syncthreads();
        for (int i = tid; i < kCols * nb; i += kThreads) {
            const int cj = blockIdx.y * kCols + i / nb;
            if (cj < a.ncols && lds[i]) atomicAdd(&a.hist[(size_t)cj * nb + i % nb], lds[i]);
        }
    }
    if (MODE == MODE_RADIX) {
        __syncthreads();
        for (int i = tid; i < kCols * kGroups * 256; i += kThreads) {
            const int cj = blockIdx.y * kCols + i / (kGroups * 256);
            const int j = (i / 256) % kGroups;
            if (cj >= a.ncols || !lds[i]) continue;
            const int n = a.ngroups[cj] - g0;
            if (j < n) atomicAdd(&a.digits[(size_t)(a.gbase[cj] + g0 + j) * 256 + (i % 256)], lds[i]);
        }
    }
}

// Σ over blocks in block order: one thread per column
__global__ void df_reduce_kernel(const double *slab, int G, int ncols, double *out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    double s = 0.0;
    for (int g = 0; g < G; g++) s = s + slab[(size_t)g * ncols + c];
    out[c] = s;
}

__global__ void df_fill_kernel(u64 *p, long long n, u64 v)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

bool ascending(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!(v[i] == v[i]) || (i && !(v[i - 1] < v[i]))) return false;
    return true;
}

}  // namespace

struct bh_datafits {
    int ncols = 0, nerr = 0, G = 1, scanned = 0;
    const double *Y = nullptr;
    const int *w = nullptr, *err = nullptr;
    long long nrows = 0, stride = 0;
    hipStream_t st = nullptr;
    u64 total = 0;
    // device
    int *wk = nullptr;
    double *slab = nullptr, *red = nullptr, *dmean = nullptr;
    u64 *kmin = nullptr, *kmax = nullptr, *cnt = nullptr;
};

namespace {

void df_free(bh_datafits *p)
{
    void *bufs[] = {p->wk, p->slab, p->red, p->dmean, p->kmin, p->kmax, p->cnt};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete p;
}

FitArgs base_args(const bh_datafits *p)
{
    FitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.Y = p->Y;
    a.nrows = p->nrows;
    a.stride = p->stride;
    a.ncols = p->ncols;
    a.wk = p->wk;
    a.slab = p->slab;
    return a;
}

template <int MODE>
int launch(bh_datafits *p, const FitArgs &a, int gz, size_t lds)
{
    dim3 grid((unsigned)p->G, (unsigned)((p->ncols + kCols - 1) / kCols), (unsigned)gz);
    hipLaunchKernelGGL((df_kernel<MODE>), grid, dim3(kThreads), lds, p->st, a);
    DF_HIP(hipGetLastError());
    return BH_OK;
}

int reduce_slab(bh_datafits *p, std::vector<double> &out)
{
    hipLaunchKernelGGL(df_reduce_kernel, dim3((unsigned)((p->ncols + 255) / 256)), dim3(256), 0, p->st,
                       (const double *)p->slab, p->G, p->ncols, p->red);
    DF_HIP(hipGetLastError());
    out.assign(p->ncols, 0.0);
    DF_HIP(hipMemcpyAsync(out.data(), p->red, sizeof(double) * p->ncols, hipMemcpyDeviceToHost, p->st));
    DF_HIP(hipStreamSynchronize(p->st));
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        bh::fail_arg_("no usable HIP device (libbayhunter_amd has no CPU fallback)");
        return BH_ERR_NO_DEVICE;
    }
    bh_datafits *p = new (std::nothrow) bh_datafits;
    if (!p) return bh::fail_arg_("out of memory");
    p->Y = Y;
    p->nrows = nrows;
    p->stride = stride;
    p->ncols = ncols;
    p->w = weights;
    p->err = err;
    p->nerr = err ? nerr : 0;
    p->st = (hipStream_t)stream;
    long long g = (nrows + kRowLanes - 1) / kRowLanes;
    p->G = (int)(g < kMaxBlocksX ? g : kMaxBlocksX);
    auto bail = [&](hipError_t e, const char *what) { df_free(p); return bh::fail_hip_((int)e, what); };
    hipError_t e;
#define DF_ALLOC(ptr, bytes) if ((e = hipMalloc((void **)&(ptr), (bytes))) != hipSuccess) return bail(e, "hipMalloc(" #ptr ")")
    DF_ALLOC(p->wk, sizeof(int) * (size_t)nrows);
    DF_ALLOC(p->slab, sizeof(double) * (size_t)p->G * ncols);
    DF_ALLOC(p->red, sizeof(double) * ncols);
    DF_ALLOC(p->dmean, sizeof(double) * ncols);
    DF_ALLOC(p->kmin, sizeof(u64) * ncols);
    DF_ALLOC(p->kmax, sizeof(u64) * ncols);
    DF_ALLOC(p->cnt, sizeof(u64) * 3);
#undef DF_ALLOC
    *fits = p;
    return BH_OK;
}

void bh_datafits_destroy(bh_datafits *fits)
{
    if (fits) {
        (void)hipStreamSynchronize(fits->st);
        df_free(fits);
    }
}

int bh_datafits_scan(bh_datafits *p, long long *total, long long *excluded, double *vmin, double *vmax,
                     double *mean)
{
    if (!p) return bh::fail_arg_("fits is NULL");
    const int N = p->ncols;
    p->scanned = 0;
    DF_HIP(hipMemsetAsync(p->cnt, 0, sizeof(u64) * 3, p->st));
    {
        long long waves = p->nrows;
        long long blocks = (waves + kThreads / 64 - 1) / (kThreads / 64);
        hipLaunchKernelGGL(df_mask_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kThreads), 0, p->st,
                           p->Y, p->nrows, p->stride, p->ncols, p->w, p->err, p->nerr, p->wk, p->cnt);
        DF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(df_fill_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, p->st, p->kmin, (long long)N, ~0ull);
    hipLaunchKernelGGL(df_fill_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, p->st, p->kmax, (long long)N, 0ull);
    DF_HIP(hipGetLastError());
    FitArgs a = base_args(p);
    a.kmin = p->kmin;
    a.kmax = p->kmax;
    int rc = launch<MODE_SCAN>(p, a, 1, 0);
    if (rc) return rc;
    u64 cnt[3];
    std::vector<u64> kmn(N), kmx(N);
    DF_HIP(hipMemcpyAsync(cnt, p->cnt, sizeof(cnt), hipMemcpyDeviceToHost, p->st));
    DF_HIP(hipMemcpyAsync(kmn.data(), p->kmin, sizeof(u64) * N, hipMemcpyDeviceToHost, p->st));
    DF_HIP(hipMemcpyAsync(kmx.data(), p->kmax, sizeof(u64) * N, hipMemcpyDeviceToHost, p->st));
    std::vector<double> sum;
    rc = reduce_slab(p, sum);                      // synchronises the stream
    if (rc) return rc;
    if (cnt[2]) return bh::fail_arg_("bh_datafits_scan: negative weight");
    if (excluded) *excluded = (long long)cnt[1];
    if (total) *total = (long long)cnt[0];
    if (cnt[0] == 0) return bh::fail_arg_("bh_datafits_scan: empty selection (no included row with a positive weight)");
    if (cnt[0] > (1ull << 53)) return bh::fail_arg_("bh_datafits_scan: weight total above 2^53");
    p->total = cnt[0];
    std::vector<double> mu(N);
    for (int c = 0; c < N; c++) mu[c] = sum[c] / (double)cnt[0];
    DF_HIP(hipMemcpyAsync(p->dmean, mu.data(), sizeof(double) * N, hipMemcpyHostToDevice, p->st));
    DF_HIP(hipStreamSynchronize(p->st));
    p->scanned = 1;
    for (int c = 0; c < N; c++) {
        if (vmin) vmin[c] = bh::post_unkey64(kmn[c]);
        if (vmax) vmax[c] = bh::post_unkey64(kmx[c]);
        if (mean) mean[c] = mu[c];
    }
    return BH_OK;
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
            if (!ascending(edges + (size_t)s * nedges, nedges)) return bh::fail_arg_("bh_datafits_finish: edges must be ascending");
    }
    if (!p) return bh::fail_arg_("fits is NULL");
    if (!p->scanned) return bh::fail_arg_("bh_datafits_finish before a successful bh_datafits_scan");
    const int N = p->ncols;
    for (int i = 0; i < nranks; i++)
        if ((u64)ranks[i] >= p->total) return bh::fail_arg_("bh_datafits_finish: rank >= the weight total");
    if (want_hist)
        for (int c = 0; c < N; c++)
            if (eset[c] < 0 || eset[c] >= nsets) return bh::fail_arg_("bh_datafits_finish: edge set out of range");

    struct Guard {
        std::vector<void *> b;
        ~Guard() { for (void *x : b) if (x) (void)hipFree(x); }
    } guard;
    const int nb = nedges - 1;
    FitArgs a = base_args(p);
    a.mean = p->dmean;
    if (stdev || want_hist) {
        size_t lds = 0;
        if (want_hist) {
            double *ded = nullptr;
            int *dset = nullptr;
            u64 *dh = nullptr;
            DF_HIP(hipMalloc((void **)&ded, sizeof(double) * (size_t)nsets * nedges));
            guard.b.push_back(ded);
            DF_HIP(hipMalloc((void **)&dset, sizeof(int) * N));
            guard.b.push_back(dset);
            DF_HIP(hipMalloc((void **)&dh, sizeof(u64) * (size_t)N * nb));
            guard.b.push_back(dh);
            DF_HIP(hipMemcpyAsync(ded, edges, sizeof(double) * (size_t)nsets * nedges, hipMemcpyHostToDevice, p->st));
            DF_HIP(hipMemcpyAsync(dset, eset, sizeof(int) * N, hipMemcpyHostToDevice, p->st));
            DF_HIP(hipMemsetAsync(dh, 0, sizeof(u64) * (size_t)N * nb, p->st));
            a.edges = ded;
            a.nedges = nedges;
            a.eset = dset;
            a.hist = dh;
            a.do_hist = 1;
            a.hist_lds = (size_t)kCols * nb * sizeof(u64) <= (size_t)kHistLdsBytes;
            lds = a.hist_lds ? (size_t)kCols * nb * sizeof(u64) : 0;
        }
        int rc = launch<MODE_FINISH>(p, a, 1, lds);
        if (rc) return rc;
        std::vector<double> sq;
        rc = reduce_slab(p, sq);                   // synchronises the stream
        if (rc) return rc;
        if (stdev)
            for (int c = 0; c < N; c++) stdev[c] = std::sqrt(sq[c] / (double)p->total);
        if (want_hist) {
            std::vector<u64> h((size_t)N * nb);
            DF_HIP(hipMemcpyAsync(h.data(), a.hist, sizeof(u64) * h.size(), hipMemcpyDeviceToHost, p->st));
            DF_HIP(hipStreamSynchronize(p->st));
            for (size_t i = 0; i < h.size(); i++) hist[i] = (long long)h[i];
        }
    }
    if (!nranks) return BH_OK;

    // radix select: per (rank, column) the prefix found so far and the rank left within it
    const size_t RN = (size_t)nranks * N;
    std::vector<u64> pfx(RN, 0), rr(RN);
    for (int i = 0; i < nranks; i++)
        for (int c = 0; c < N; c++) rr[(size_t)i * N + c] = (u64)ranks[i];
    int *dgb = nullptr, *dng = nullptr;
    u64 *dgp = nullptr, *ddig = nullptr;
    DF_HIP(hipMalloc((void **)&dgb, sizeof(int) * N));
    guard.b.push_back(dgb);
    DF_HIP(hipMalloc((void **)&dng, sizeof(int) * N));
    guard.b.push_back(dng);
    DF_HIP(hipMalloc((void **)&dgp, sizeof(u64) * RN));
    guard.b.push_back(dgp);
    DF_HIP(hipMalloc((void **)&ddig, sizeof(u64) * 256 * RN));
    guard.b.push_back(ddig);
    std::vector<int> gb(N), ngr(N), grp(RN);        // grp: the group (slot) of each (rank, column)
    std::vector<u64> gp(RN), dig;
    for (int shift = 56; shift >= 0; shift -= 8) {
        // groups: distinct prefixes of the column's ranks
        int slots = 0, maxg = 0;
        for (int c = 0; c < N; c++) {
            gb[c] = slots;
            int n = 0;
            for (int i = 0; i < nranks; i++) {
                const u64 v = pfx[(size_t)i * N + c];
                int j = 0;
                while (j < n && gp[slots + j] != v) j++;
                if (j == n) gp[slots + n++] = v;
                grp[(size_t)i * N + c] = slots + j;
            }
            ngr[c] = n;
            slots += n;
            maxg = n > maxg ? n : maxg;
        }
        DF_HIP(hipMemcpyAsync(dgb, gb.data(), sizeof(int) * N, hipMemcpyHostToDevice, p->st));
        DF_HIP(hipMemcpyAsync(dng, ngr.data(), sizeof(int) * N, hipMemcpyHostToDevice, p->st));
        DF_HIP(hipMemcpyAsync(dgp, gp.data(), sizeof(u64) * slots, hipMemcpyHostToDevice, p->st));
        DF_HIP(hipMemsetAsync(ddig, 0, sizeof(u64) * 256 * (size_t)slots, p->st));
        FitArgs r = base_args(p);
        r.shift = shift;
        r.gbase = dgb;
        r.ngroups = dng;
        r.gpfx = dgp;
        r.digits = ddig;
        int rc = launch<MODE_RADIX>(p, r, (maxg + kGroups - 1) / kGroups, sizeof(u64) * kCols * kGroups * 256);
        if (rc) return rc;
        dig.resize((size_t)slots * 256);
        DF_HIP(hipMemcpyAsync(dig.data(), ddig, sizeof(u64) * dig.size(), hipMemcpyDeviceToHost, p->st));
        DF_HIP(hipStreamSynchronize(p->st));
        for (size_t i = 0; i < RN; i++) {
            const u64 *h = &dig[(size_t)grp[i] * 256];
            u64 left = rr[i], cum = 0;
            int b = 0;
            for (; b < 255 && cum + h[b] <= left; b++) cum += h[b];
            pfx[i] = (pfx[i] << 8) | (u64)b;
            rr[i] = left - cum;
        }
    }
    for (size_t i = 0; i < RN; i++) order_stats[i] = bh::post_unkey64(pfx[i]);
    return BH_OK;
}

}  // extern "C"
