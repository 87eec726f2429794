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
//   sens_sets_fold_kernel   (sens_sets_host.h, with nw = nper weight pairs a block) one thread per item, and one per
//                           period for the weights, adds the slab's rows to their sets' sums in block order.
//
// The slab holds a bounded number of blocks: a call's blocks are taken in chunks, each folded before the next is
// launched, which is the order of one pass over all of them.  The handle, that loop and the finish are
// sens_sets_host.h's SensSetsHandle; here are the main kernel, its arguments and launch, and the checks of what only
// this reduction takes.  No scratch; LDS sens_sets_lds_doubles (49 KiB at 100 layers and 60 periods).
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

typedef bh::SensSetsHandle SensSets;    // nw = nper: a block carries a weight pair per period

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
    s->init(set_start, nsets, edges, nedges, kind, drho_dvp, stream);
    s->nw = nper;
    s->nitems = (size_t)nper * nedges;
    if (int rc = s->make_ready()) {
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
    if (int rc = s->check_add(who, row0, B, Lmax, model_stride, nlay, hthk, q, q_stride, K, c_out ? nullptr : "NULL pointer"))
        return rc;
    if (B == 0) return BH_OK;
    const int nper = s->nw;
    SensSetsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.blocks = s->dblocks;
    a.Lmax = Lmax; a.mstride = model_stride; a.qstride = q_stride; a.nper = nper; a.nb = s->nb; a.kind = s->kind;
    a.span = bh::sens_sets_span(nper, s->nb);
    a.drho = s->drho;
    a.nlay = nlay; a.w = weights; a.h = hthk; a.q = q; a.K = K; a.c = c_out; a.edges = s->dedges;
    a.slab = s->slab; a.wslab = s->wslab; a.neg = s->neg;
    const size_t lds = sizeof(double) * (size_t)bh::sens_sets_lds_doubles(Lmax, nper, s->nb);
    const unsigned groups = (unsigned)(((int)s->nitems + kSensSetsThreads - 1) / kSensSetsThreads);
    return s->add(who, row0, B, [&](unsigned nblocks) {
        hipLaunchKernelGGL(sens_sets_kernel, dim3(nblocks, groups), dim3(kSensSetsThreads), lds, s->st, a);
    });
}

extern "C" int bh_sens_sets_finish(void *handle, long long *total, long long *excluded, double *s1, double *s2,
                                   double *vmin, double *vmax)
{
    const char *who = "bh_sens_sets_finish";
    if (!handle) return bh::fail_who(who, "handle is NULL");
    return ((SensSets *)handle)->finish(who, total, excluded, s1, s2, vmin, vmax);
}

extern "C" void bh_sens_sets_destroy(void *handle)
{
    delete (SensSets *)handle;
}
