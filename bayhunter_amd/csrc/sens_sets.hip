// sens_sets.hip -- depth-binned sensitivity kernels of many sets of weighted rows (bh_sens_sets_*): per set, period and
// depth cell the first two moments, the minimum and the maximum of dc/dm spread over shared depth bins.  The definitions
// and the order of the sums are in sens_sets_core.h.
//
//   sens_sets_kernel        a workgroup takes one block of a set's rows (the host lists the blocks) and one group of
//                           kSensSetsThreads items (period, cell), one per thread.  Per row the workgroup stages the
//                           thicknesses, c_out and the layer values G of the periods its items touch in LDS -- K is read
//                           once per group, the kinds that enter G only --, one thread forms the tops from LDS, and every
//                           thread walks the row's layers for its cell and feeds its chain.  The weight, nlay and the row
//                           index are uniform in the workgroup: a row without weight or without a model costs no barrier.
//                           The partial goes to the block's row of the slab; the thread of cell 0 of a period also
//                           carries the period's total and excluded weight.
//   sens_sets_fold_kernel   one thread per item (and one per period for the weights) adds the slab's rows to their sets'
//                           sums in block order.
//
// The slab holds a bounded number of blocks: a call's blocks are taken in chunks, each folded before the next is
// launched, which is the order of one pass over all of them.  No scratch; LDS sens_sets_lds_doubles (49 KiB at 100
// layers and 60 periods).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "sens_sets_core.h"
#include "sens_sets_host.h"

namespace {

using bh::u64;
using bh::SensSetsAcc;
using bh::kSensSetsThreads;

struct SensSetsArgs {
    const int3 *blocks;                // [grid.x]: (set, first row within the call, rows)
    int Lmax, mstride, qstride, nper, nb, kind, span;
    double drho;
    const int *nlay, *w;
    const double *h, *q, *K, *c, *edges;
    SensSetsAcc *slab;                 // [grid.x][nper * (nb + 1)]
    long long *wslab;                  // [grid.x][nper][2]: total, excluded
    u64 *neg;                          // rows with a negative weight
};

__global__ __launch_bounds__(kSensSetsThreads) void sens_sets_kernel(SensSetsArgs a)
{
    extern __shared__ double lds[];
    double *hh = lds, *tops = hh + a.Lmax, *cc = tops + a.Lmax, *G = cc + a.span;     // G [span][Lmax]
    const int tid = threadIdx.x, cells = a.nb + 1, nitems = a.nper * cells;
    const int first = blockIdx.y * kSensSetsThreads;
    const int last = first + kSensSetsThreads - 1 < nitems ? first + kSensSetsThreads - 1 : nitems - 1;
    const int p0 = first / cells, np = last / cells - p0 + 1;                         // np <= span
    const int item = first + tid;
    const bool live = item < nitems;
    const int p = live ? item / cells : p0, j = live ? item - p * cells : 0;
    const bool weighs = live && j == 0;
    const int3 blk = a.blocks[blockIdx.x];
    SensSetsAcc acc;
    bh::sens_sets_acc_init(acc);
    long long tot = 0, exc = 0;
    for (int i = 0; i < blk.z; i++) {
        const long long r = (long long)blk.y + i;
        const int w = a.w ? a.w[r] : 1;
        if (w <= 0) {
            if (w < 0 && tid == 0 && blockIdx.y == 0) atomicAdd(a.neg, (u64)1);
            continue;
        }
        const int nl = a.nlay[r];
        if (nl < 2 || nl > a.Lmax) {
            if (weighs) exc += w;
            continue;
        }
        __syncthreads();                               // the row before has been read
        const double *hrow = a.h + r * a.mstride, *qrow = a.q ? a.q + r * a.qstride : nullptr;
        const double *Krow = a.K + (r * a.nper + p0) * 4 * a.Lmax;
        for (int k = tid; k < nl; k += kSensSetsThreads) hh[k] = hrow[k];
        for (int k = tid; k < np; k += kSensSetsThreads) cc[k] = a.c[r * a.nper + p0 + k];
        for (int k = tid; k < np * nl; k += kSensSetsThreads) {
            const int pp = k / nl, l = k - pp * nl;
            G[pp * a.Lmax + l] = bh::sens_sets_layer(a.kind, a.drho, Krow + (size_t)pp * 4 * a.Lmax, a.Lmax, qrow, l);
        }
        __syncthreads();
        if (tid == 0) bh::sens_sets_tops(hh, nl, tops);
        __syncthreads();
        if (live) {
            if (bh::sens_sets_counts(w, nl, a.Lmax, cc[p - p0])) {
                const double x = bh::sens_sets_cell(tops, hh, G + (p - p0) * a.Lmax, nl, a.edges, a.nb, j);
                bh::sens_sets_acc_row(acc, (double)w, x);
                if (weighs) tot += w;
            } else if (weighs) {
                exc += w;
            }
        }
    }
    if (live) a.slab[(size_t)blockIdx.x * nitems + item] = acc;
    if (weighs) {
        long long *out = a.wslab + ((size_t)blockIdx.x * a.nper + p) * 2;
        out[0] = tot;
        out[1] = exc;
    }
}

// thread t < nitems: item t of every block's partial into its set's sums; the next nper threads: the weights
__global__ void sens_sets_fold_kernel(const int3 *blocks, int nblocks, int nitems, int nper, const SensSetsAcc *slab,
                                      const long long *wslab, SensSetsAcc *acc, long long *wacc)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nitems) {
        int z = -1;
        SensSetsAcc cur;
        bh::sens_sets_acc_init(cur);
        for (int b = 0; b < nblocks; b++) {
            const int zb = blocks[b].x;
            if (zb != z) {
                if (z >= 0) acc[(size_t)z * nitems + t] = cur;
                z = zb;
                cur = acc[(size_t)z * nitems + t];
            }
            bh::sens_sets_acc_fold(cur, slab[(size_t)b * nitems + t]);
        }
        if (z >= 0) acc[(size_t)z * nitems + t] = cur;
    } else if (t < nitems + nper) {
        const int p = t - nitems;
        for (int b = 0; b < nblocks; b++) {
            long long *out = wacc + ((size_t)blocks[b].x * nper + p) * 2;
            out[0] += wslab[((size_t)b * nper + p) * 2];
            out[1] += wslab[((size_t)b * nper + p) * 2 + 1];
        }
    }
}

__global__ void sens_sets_init_kernel(SensSetsAcc *acc, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bh::sens_sets_acc_init(acc[i]);
}

struct SensSets {
    int nsets = 0, nper = 0, nb = 0, kind = 0;
    double drho = 0.0;
    hipStream_t st = nullptr;
    bh::SensSetRows rows;                          // the sets, and the row the next add begins with
    size_t cap = 1;                                // blocks the slab holds
    bh::DevBufs bufs;
    double *dedges = nullptr;
    int3 *dblocks = nullptr;
    SensSetsAcc *slab = nullptr, *acc = nullptr;   // [cap][nitems], [nsets][nitems]
    long long *wslab = nullptr, *wacc = nullptr;   // [cap][nper][2], [nsets][nper][2]
    u64 *neg = nullptr;

    size_t nitems() const { return (size_t)nper * (nb + 1); }
};

int create(SensSets *s, const double *edges, int nedges)
{
    const size_t n = s->nitems();
    s->cap = s->rows.slab_blocks(n);
    BH_HIP(s->bufs.alloc(s->dedges, (size_t)nedges));
    BH_HIP(s->bufs.alloc(s->dblocks, s->cap));
    BH_HIP(s->bufs.alloc(s->slab, s->cap * n));
    BH_HIP(s->bufs.alloc(s->wslab, s->cap * s->nper * 2));
    BH_HIP(s->bufs.alloc(s->acc, (size_t)s->nsets * n));
    BH_HIP(s->bufs.alloc(s->wacc, (size_t)s->nsets * s->nper * 2));
    BH_HIP(s->bufs.alloc(s->neg, 1));
    BH_HIP(hipMemcpyAsync(s->dedges, edges, sizeof(double) * nedges, hipMemcpyHostToDevice, s->st));
    BH_HIP(hipMemsetAsync(s->wacc, 0, sizeof(long long) * (size_t)s->nsets * s->nper * 2, s->st));
    BH_HIP(hipMemsetAsync(s->neg, 0, sizeof(u64), s->st));
    const size_t cells = (size_t)s->nsets * n;
    hipLaunchKernelGGL(sens_sets_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s->st, s->acc, cells);
    BH_HIP(hipGetLastError());
    BH_HIP(hipStreamSynchronize(s->st));           // `edges` is the caller's
    return BH_OK;
}

}  // namespace

extern "C" int bh_sens_sets_create(void **handle, const long long *set_start, int nsets, int nper, const double *edges,
                                   int nedges, int kind, double drho_dvp, void *stream)
{
    const char *who = "bh_sens_sets_create";
    if (int rc = bh::sens_sets_check_sets(who, handle, set_start, nsets)) return rc;
    if (nper < 1 || nper > BH_MAX_PERIODS) return bh::fail_who(who, "nper out of range (1 .. 60)");
    if (int rc = bh::sens_sets_check_grid(who, edges, nedges, kind, drho_dvp)) return rc;
    if (int rc = bh::require_device()) return rc;
    SensSets *s = new (std::nothrow) SensSets;
    if (!s) return bh::fail_who(who, "out of host memory");
    s->nsets = nsets;
    s->nper = nper;
    s->nb = nedges - 1;
    s->kind = kind;
    s->drho = drho_dvp;
    s->st = (hipStream_t)stream;
    s->rows.nsets = nsets;
    s->rows.start.assign(set_start, set_start + nsets + 1);
    if (int rc = create(s, edges, nedges)) {
        delete s;
        return rc;
    }
    *handle = s;
    return BH_OK;
}

extern "C" int bh_sens_sets_add(void *handle, long long row0, int B, int Lmax, int model_stride, const int *nlay,
                                const double *hthk, const double *q, int q_stride, const double *K, const double *c_out,
                                const int *weights)
{
    const char *who = "bh_sens_sets_add";
    SensSets *s = (SensSets *)handle;
    if (!s) return bh::fail_who(who, "handle is NULL");
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return bh::fail_who(who, "B/Lmax out of range");
    if (model_stride < Lmax) return bh::fail_who(who, "model_stride < Lmax");
    if (const char *fault = bh::sens_sets_rows_fault(s->rows, row0, B)) return bh::fail_who(who, fault);
    if (B == 0) return BH_OK;
    if (s->kind == BH_SENS_KIND_VS_TOTAL && !q) return bh::fail_who(who, "BH_SENS_KIND_VS_TOTAL needs q");
    if (q && q_stride < Lmax) return bh::fail_who(who, "q_stride < Lmax");
    if (!nlay || !hthk || !K || !c_out) return bh::fail_who(who, "NULL pointer");
    if (!s->rows.cut_ok(row0) || !s->rows.cut_ok(row0 + B)) return bh::fail_who(who, bh::kSensSetsCutFault);
    std::vector<int3> blocks;
    bh::CallBufs drain(s->st);                      // (owns nothing: an early return waits for the copies of `blocks`)
    s->rows.call_blocks(row0, B, blocks);
    SensSetsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.blocks = s->dblocks;
    a.Lmax = Lmax; a.mstride = model_stride; a.qstride = q_stride; a.nper = s->nper; a.nb = s->nb; a.kind = s->kind;
    a.span = bh::sens_sets_span(s->nper, s->nb);
    a.drho = s->drho;
    a.nlay = nlay; a.w = weights; a.h = hthk; a.q = q; a.K = K; a.c = c_out; a.edges = s->dedges;
    a.slab = s->slab; a.wslab = s->wslab; a.neg = s->neg;
    const size_t lds = sizeof(double) * (size_t)bh::sens_sets_lds_doubles(Lmax, s->nper, s->nb);
    const int nitems = (int)s->nitems();
    const unsigned groups = (unsigned)((nitems + kSensSetsThreads - 1) / kSensSetsThreads);
    const unsigned fold = (unsigned)((nitems + s->nper + 255) / 256);
    for (size_t b0 = 0; b0 < blocks.size(); b0 += s->cap) {
        const size_t nb = blocks.size() - b0 < s->cap ? blocks.size() - b0 : s->cap;
        BH_HIP(hipMemcpyAsync(s->dblocks, blocks.data() + b0, sizeof(int3) * nb, hipMemcpyHostToDevice, s->st));
        hipLaunchKernelGGL(sens_sets_kernel, dim3((unsigned)nb, groups), dim3(kSensSetsThreads), lds, s->st, a);
        BH_HIP(hipGetLastError());
        hipLaunchKernelGGL(sens_sets_fold_kernel, dim3(fold), dim3(256), 0, s->st, (const int3 *)s->dblocks, (int)nb, nitems,
                           s->nper, (const SensSetsAcc *)s->slab, (const long long *)s->wslab, s->acc, s->wacc);
        BH_HIP(hipGetLastError());
    }
    // the call's arrays are free when it returns, and a negative weight is reported by the call that brought it
    u64 bad = 0;
    BH_HIP(hipMemcpyAsync(&bad, s->neg, sizeof(u64), hipMemcpyDeviceToHost, s->st));
    BH_HIP(hipStreamSynchronize(s->st));
    s->rows.next = row0 + B;
    if (bad) return bh::fail_who(who, "negative weight");
    return BH_OK;
}

extern "C" int bh_sens_sets_finish(void *handle, long long *total, long long *excluded, double *s1, double *s2,
                                   double *vmin, double *vmax)
{
    const char *who = "bh_sens_sets_finish";
    SensSets *s = (SensSets *)handle;
    if (!s) return bh::fail_who(who, "handle is NULL");
    if (s->rows.next != s->rows.total_rows()) return bh::fail_who(who, "not all rows of set_start were added");
    const size_t n = s->nitems(), cells = (size_t)s->nsets * n, nw = (size_t)s->nsets * s->nper;
    std::vector<SensSetsAcc> acc(cells);
    std::vector<long long> wacc(nw * 2);
    u64 bad = 0;
    BH_HIP(hipMemcpyAsync(acc.data(), s->acc, sizeof(SensSetsAcc) * cells, hipMemcpyDeviceToHost, s->st));
    BH_HIP(hipMemcpyAsync(wacc.data(), s->wacc, sizeof(long long) * nw * 2, hipMemcpyDeviceToHost, s->st));
    BH_HIP(hipMemcpyAsync(&bad, s->neg, sizeof(u64), hipMemcpyDeviceToHost, s->st));
    BH_HIP(hipStreamSynchronize(s->st));
    if (bad) return bh::fail_who(who, "negative weight");
    const double nan = std::nan("");
    for (size_t zp = 0; zp < nw; zp++) {
        const bool any = wacc[2 * zp] > 0;             // a period without a row that counts: sums 0, min / max NaN
        if (total) total[zp] = wacc[2 * zp];
        if (excluded) excluded[zp] = wacc[2 * zp + 1];
        for (size_t j = 0; j <= (size_t)s->nb; j++) {
            const size_t i = zp * (s->nb + 1) + j;
            if (s1) s1[i] = any ? acc[i].s1 : 0.0;
            if (s2) s2[i] = any ? acc[i].s2 : 0.0;
            if (vmin) vmin[i] = any ? acc[i].vmin : nan;
            if (vmax) vmax[i] = any ? acc[i].vmax : nan;
        }
    }
    return BH_OK;
}

extern "C" void bh_sens_sets_destroy(void *handle)
{
    SensSets *s = (SensSets *)handle;
    if (!s) return;
    (void)hipStreamSynchronize(s->st);
    delete s;
}
