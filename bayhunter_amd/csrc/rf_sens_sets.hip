// rf_sens_sets.hip -- depth-binned receiver-function sensitivity kernels of many sets of weighted rows
// (bh_rf_sens_sets_*): per set, selected sample of the trace and depth cell the first two moments, the minimum and the
// maximum of dRF(t)/dm spread over shared depth bins.  The definitions and the order of the sums are in sens_sets_core.h,
// the tile and the per-thread body in rf_sens_sets_core.h.
//
//   rf_sens_sets_kernel        a workgroup takes one block of a set's rows (the host lists the blocks) and a tile of
//                              kRfSensSetsCells cells x kRfSensSetsTileSamples selected samples.  A thread owns one cell
//                              and kRfSensSetsRS samples, with one accumulator of four doubles per sample.  Per row the
//                              workgroup stages the thicknesses and the layer values G[l][sample] of the tile's samples in
//                              LDS -- K is read at the selected samples and at the kinds that enter G only --, one thread
//                              forms the tops, and every thread walks the row's layers once for its cell: d / h_l once
//                              per overlapping layer, applied to its chains.  The weight, nlay, the row index and the
//                              trace's first sample are uniform in the workgroup: a row that does not count costs no
//                              barrier.  The partials go to the block's row of the slab; thread 0 of tile 0 carries the
//                              block's total and excluded weight.
//   rf_sens_sets_fold_kernel   one thread per item (and one for the weights) adds the slab's rows to their sets' sums in
//                              block order.
//
// The slab holds a bounded number of blocks: a call's blocks are taken in chunks, each folded before the next is
// launched, which is the order of one pass over all of them.  create checks and records; the device is first touched by
// the first add that brings rows, after all of that call's arguments were checked.  No scratch; LDS
// rf_sens_sets_lds_doubles and the tile's sample offsets (14 464 B at 100 layers).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "rf_sens_sets_core.h"
#include "sens_sets_host.h"

namespace {

using bh::u64;
using bh::SensSetsAcc;
constexpr int kThreads = bh::kRfSensSetsThreads, kRS = bh::kRfSensSetsRS, kCells = bh::kRfSensSetsCells;
constexpr int kTileSamples = bh::kRfSensSetsTileSamples;

struct RfSensSetsArgs {
    const int3 *blocks;                // [grid.x]: (set, first row within the call, rows)
    int Lmax, mstride, qstride, rfstride, nsel, nb, kind, ctiles;
    long long kstride;
    double drho;
    const int *nlay, *w, *samples;     // samples [nsel]: the selected samples of K's nout
    const double *h, *q, *K, *rf, *edges;
    SensSetsAcc *slab;                 // [grid.x][nsel * (nb + 1)]
    long long *wslab;                  // [grid.x][2]: total, excluded
    u64 *neg;                          // rows with a negative weight
};

size_t lds_bytes(int Lmax) { return sizeof(double) * (size_t)bh::rf_sens_sets_lds_doubles(Lmax) + sizeof(int) * kTileSamples; }

// Four waves a SIMD, 128 VGPRs.  With kRfSensSetsRS = 8 the kernel took 166 VGPRs left alone and spilled 100 bytes under
// this bound (the accumulators alone are 64); with 4 it takes 89 and spills nothing.
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void rf_sens_sets_kernel(RfSensSetsArgs a)
{
    extern __shared__ double lds[];
    double *hh = lds, *tops = hh + a.Lmax, *G = tops + a.Lmax;                         // G [Lmax][kTileSamples]
    int *koff = (int *)(G + kTileSamples * a.Lmax);                                    // [kTileSamples] sample * 4 * Lmax
    const int tid = threadIdx.x, cells = a.nb + 1;
    const int ct = blockIdx.y % a.ctiles, stile = blockIdx.y / a.ctiles;
    const int j = ct * kCells + tid % kCells;                                          // the thread's cell
    const int t0 = stile * kTileSamples;                                               // the tile's first selected sample
    const int nt = a.nsel - t0 < kTileSamples ? a.nsel - t0 : kTileSamples;            // its samples
    const int s0 = tid / kCells * kRS;                                                 // the thread's first, in the tile
    const bool live = j < cells && s0 < nt, half = j == a.nb;
    const bool weighs = blockIdx.y == 0 && tid == 0;
    const double e0 = j < a.nb ? a.edges[j] : 0.0, e1 = j < a.nb ? a.edges[j + 1] : 0.0;
    if (tid < nt) koff[tid] = a.samples[t0 + tid] * 4 * a.Lmax;
    if (nt < kTileSamples)                                                             // samples the tile has not: 0
        for (int k = tid; k < kTileSamples * a.Lmax; k += kThreads) G[k] = 0.0;
    const int3 blk = a.blocks[blockIdx.x];
    SensSetsAcc acc[kRS];
#pragma unroll
    for (int s = 0; s < kRS; s++) bh::sens_sets_acc_init(acc[s]);
    long long tot = 0, exc = 0;
    for (int i = 0; i < blk.z; i++) {
        const long long r = (long long)blk.y + i;
        const int w = a.w ? a.w[r] : 1;
        if (w <= 0) {
            if (w < 0 && weighs) atomicAdd(a.neg, (u64)1);
            continue;
        }
        const int nl = a.nlay[r];
        if (!bh::rf_sens_sets_counts(w, nl, a.Lmax, nl >= 2 && nl <= a.Lmax ? a.rf[r * a.rfstride] : 0.0)) {
            if (weighs) exc += w;
            continue;
        }
        if (weighs) tot += w;
        __syncthreads();                               // the row before has been read (and koff is there)
        const double *hrow = a.h + r * a.mstride, *qrow = a.q ? a.q + r * a.qstride : nullptr;
        const double *Krow = a.K + r * a.kstride;
        if (tid == kThreads - 1) bh::sens_sets_tops(hrow, nl, tops);
        for (int k = tid; k < nl; k += kThreads) hh[k] = hrow[k];
#pragma unroll 2
        for (int k = tid; k < nt * nl; k += kThreads) {
            const int s = k / nl, l = k - s * nl;
            G[l * kTileSamples + s] = bh::sens_sets_layer(a.kind, a.drho, Krow + koff[s], a.Lmax, qrow, l);
        }
        __syncthreads();
        if (live) {
            double x[kRS];
            bh::rf_sens_sets_cells<kRS>(tops, hh, G + s0, kTileSamples, nl, e0, e1, half, x);
            bh::rf_sens_sets_acc_rows<kRS>(acc, (double)w, x);
        }
    }
    if (live) {
        SensSetsAcc *out = a.slab + (size_t)blockIdx.x * a.nsel * cells + (size_t)(t0 + s0) * cells + j;
#pragma unroll
        for (int s = 0; s < kRS; s++)
            if (s0 + s < nt) out[(size_t)s * cells] = acc[s];
    }
    if (weighs) {
        a.wslab[(size_t)blockIdx.x * 2] = tot;
        a.wslab[(size_t)blockIdx.x * 2 + 1] = exc;
    }
}

// thread t < nitems: item t of every block's partial into its set's sums; thread nitems: the weights
__global__ void rf_sens_sets_fold_kernel(const int3 *blocks, int nblocks, int nitems, const SensSetsAcc *slab,
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
    } else if (t == nitems) {
        for (int b = 0; b < nblocks; b++) {
            long long *out = wacc + (size_t)blocks[b].x * 2;
            out[0] += wslab[(size_t)b * 2];
            out[1] += wslab[(size_t)b * 2 + 1];
        }
    }
}

__global__ void rf_sens_sets_init_kernel(SensSetsAcc *acc, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bh::sens_sets_acc_init(acc[i]);
}

struct RfSensSets {
    int nsets = 0, nout = 0, nsel = 0, nb = 0, kind = 0;
    double drho = 0.0;
    hipStream_t st = nullptr;
    bh::SensSetRows rows;                          // the sets, and the row the next add begins with
    std::vector<int> samples;                      // [nsel]
    std::vector<double> edges;                     // [nb + 1]
    bool ready = false;                            // the device buffers are there
    size_t cap = 1;                                // blocks the slab holds
    bh::DevBufs bufs;
    double *dedges = nullptr;
    int *dsamples = nullptr;
    int3 *dblocks = nullptr;
    SensSetsAcc *slab = nullptr, *acc = nullptr;   // [cap][nitems], [nsets][nitems]
    long long *wslab = nullptr, *wacc = nullptr;   // [cap][2], [nsets][2]
    u64 *neg = nullptr;

    size_t nitems() const { return (size_t)nsel * (nb + 1); }
};

// the first add that brings rows: the device, the buffers, the accumulators at their start
int make_ready(RfSensSets *s)
{
    if (s->ready) return BH_OK;
    if (int rc = bh::require_device()) return rc;
    const size_t n = s->nitems(), cells = (size_t)s->nsets * n;
    s->cap = s->rows.slab_blocks(n);
    BH_HIP(s->bufs.alloc(s->dedges, s->edges.size()));
    BH_HIP(s->bufs.alloc(s->dsamples, (size_t)s->nsel));
    BH_HIP(s->bufs.alloc(s->dblocks, s->cap));
    BH_HIP(s->bufs.alloc(s->slab, s->cap * n));
    BH_HIP(s->bufs.alloc(s->wslab, s->cap * 2));
    BH_HIP(s->bufs.alloc(s->acc, cells));
    BH_HIP(s->bufs.alloc(s->wacc, (size_t)s->nsets * 2));
    BH_HIP(s->bufs.alloc(s->neg, 1));
    BH_HIP(hipMemcpyAsync(s->dedges, s->edges.data(), sizeof(double) * s->edges.size(), hipMemcpyHostToDevice, s->st));
    BH_HIP(hipMemcpyAsync(s->dsamples, s->samples.data(), sizeof(int) * s->nsel, hipMemcpyHostToDevice, s->st));
    BH_HIP(hipMemsetAsync(s->wacc, 0, sizeof(long long) * (size_t)s->nsets * 2, s->st));
    BH_HIP(hipMemsetAsync(s->neg, 0, sizeof(u64), s->st));
    hipLaunchKernelGGL(rf_sens_sets_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s->st, s->acc, cells);
    BH_HIP(hipGetLastError());
    s->ready = true;
    return BH_OK;
}

}  // namespace

extern "C" int bh_rf_sens_sets_create(void **handle, const long long *set_start, int nsets, int nout, const int *samples,
                                      int nsel, const double *edges, int nedges, int kind, double drho_dvp, void *stream)
{
    const char *who = "bh_rf_sens_sets_create";
    if (int rc = bh::sens_sets_check_sets(who, handle, set_start, nsets)) return rc;
    if (nout < 1 || nout > BH_RF_SENS_SETS_MAX_SAMPLES) return bh::fail_who(who, "nout out of range (1 .. 4096)");
    if (samples) {
        if (nsel < 1 || nsel > nout) return bh::fail_who(who, "nsel out of range (1 .. nout)");
        for (int i = 0; i < nsel; i++) {
            if (samples[i] < 0 || samples[i] >= nout) return bh::fail_who(who, "sample index out of range (0 .. nout - 1)");
            if (i && samples[i] <= samples[i - 1]) return bh::fail_who(who, "sample indices must be strictly ascending");
        }
    } else {
        nsel = nout;
    }
    if (int rc = bh::sens_sets_check_grid(who, edges, nedges, kind, drho_dvp)) return rc;
    if ((long long)nsets * nsel * nedges * (long long)sizeof(SensSetsAcc) > BH_RF_SENS_SETS_MAX_ACC_BYTES)
        return bh::fail_who(who, "the accumulators, nsets * nsel * (nb + 1) * 32 bytes, exceed "
                                 "BH_RF_SENS_SETS_MAX_ACC_BYTES: fewer samples or sets a handle");
    RfSensSets *s = new (std::nothrow) RfSensSets;
    if (!s) return bh::fail_who(who, "out of host memory");
    s->nsets = nsets;
    s->nout = nout;
    s->nsel = nsel;
    s->nb = nedges - 1;
    s->kind = kind;
    s->drho = drho_dvp;
    s->st = (hipStream_t)stream;
    s->rows.nsets = nsets;
    s->rows.start.assign(set_start, set_start + nsets + 1);
    s->edges.assign(edges, edges + nedges);
    s->samples.resize(nsel);
    for (int i = 0; i < nsel; i++) s->samples[i] = samples ? samples[i] : i;
    *handle = s;
    return BH_OK;
}

extern "C" int bh_rf_sens_sets_add(void *handle, long long row0, int B, int Lmax, int model_stride, const int *nlay,
                                   const double *hthk, const double *q, int q_stride, const double *K, long long k_stride,
                                   const double *rf, int rf_stride, const int *weights)
{
    const char *who = "bh_rf_sens_sets_add";
    RfSensSets *s = (RfSensSets *)handle;
    if (!s) return bh::fail_who(who, "handle is NULL");
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return bh::fail_who(who, "B/Lmax out of range");
    if (model_stride < Lmax) return bh::fail_who(who, "model_stride < Lmax");
    if (const char *fault = bh::sens_sets_rows_fault(s->rows, row0, B)) return bh::fail_who(who, fault);
    if (B == 0) return BH_OK;
    if (s->kind == BH_SENS_KIND_VS_TOTAL && !q) return bh::fail_who(who, "BH_SENS_KIND_VS_TOTAL needs q");
    if (q && q_stride < Lmax) return bh::fail_who(who, "q_stride < Lmax");
    if (!nlay || !hthk || !K || !rf) return bh::fail_who(who, "NULL pointer");
    if (k_stride < (long long)s->nout * 4 * Lmax) return bh::fail_who(who, "k_stride < nout * 4 * Lmax");
    if (rf_stride < s->nout) return bh::fail_who(who, "rf_stride < nout");
    if (!s->rows.cut_ok(row0) || !s->rows.cut_ok(row0 + B)) return bh::fail_who(who, bh::kSensSetsCutFault);
    if (int rc = make_ready(s)) return rc;
    std::vector<int3> blocks;
    bh::CallBufs drain(s->st);                      // (owns nothing: an early return waits for the copies of `blocks`)
    s->rows.call_blocks(row0, B, blocks);
    RfSensSetsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.blocks = s->dblocks;
    a.Lmax = Lmax; a.mstride = model_stride; a.qstride = q_stride; a.rfstride = rf_stride; a.nsel = s->nsel; a.nb = s->nb;
    a.kind = s->kind; a.ctiles = bh::rf_sens_sets_cell_tiles(s->nb);
    a.kstride = k_stride;
    a.drho = s->drho;
    a.nlay = nlay; a.w = weights; a.samples = s->dsamples; a.h = hthk; a.q = q; a.K = K; a.rf = rf; a.edges = s->dedges;
    a.slab = s->slab; a.wslab = s->wslab; a.neg = s->neg;
    const int nitems = (int)s->nitems();
    const unsigned tiles = (unsigned)(a.ctiles * bh::rf_sens_sets_sample_tiles(s->nsel));
    const unsigned fold = (unsigned)((nitems + 1 + 255) / 256);
    for (size_t b0 = 0; b0 < blocks.size(); b0 += s->cap) {
        const size_t nb = blocks.size() - b0 < s->cap ? blocks.size() - b0 : s->cap;
        BH_HIP(hipMemcpyAsync(s->dblocks, blocks.data() + b0, sizeof(int3) * nb, hipMemcpyHostToDevice, s->st));
        hipLaunchKernelGGL(rf_sens_sets_kernel, dim3((unsigned)nb, tiles), dim3(kThreads), lds_bytes(Lmax), s->st, a);
        BH_HIP(hipGetLastError());
        hipLaunchKernelGGL(rf_sens_sets_fold_kernel, dim3(fold), dim3(256), 0, s->st, (const int3 *)s->dblocks, (int)nb,
                           nitems, (const SensSetsAcc *)s->slab, (const long long *)s->wslab, s->acc, s->wacc);
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

extern "C" int bh_rf_sens_sets_finish(void *handle, long long *total, long long *excluded, double *s1, double *s2,
                                      double *vmin, double *vmax)
{
    const char *who = "bh_rf_sens_sets_finish";
    RfSensSets *s = (RfSensSets *)handle;
    if (!s) return bh::fail_who(who, "handle is NULL");
    if (s->rows.next != s->rows.total_rows()) return bh::fail_who(who, "not all rows of set_start were added");
    const size_t n = s->nitems(), cells = (size_t)s->nsets * n;
    std::vector<SensSetsAcc> acc;
    std::vector<long long> wacc((size_t)s->nsets * 2, 0);
    if (s->ready) {                                 // (not ready: no set has a row)
        u64 bad = 0;
        acc.resize(cells);
        BH_HIP(hipMemcpyAsync(acc.data(), s->acc, sizeof(SensSetsAcc) * cells, hipMemcpyDeviceToHost, s->st));
        BH_HIP(hipMemcpyAsync(wacc.data(), s->wacc, sizeof(long long) * wacc.size(), hipMemcpyDeviceToHost, s->st));
        BH_HIP(hipMemcpyAsync(&bad, s->neg, sizeof(u64), hipMemcpyDeviceToHost, s->st));
        BH_HIP(hipStreamSynchronize(s->st));
        if (bad) return bh::fail_who(who, "negative weight");
    }
    const double nan = std::nan("");
    for (size_t z = 0; z < (size_t)s->nsets; z++) {
        const bool any = wacc[2 * z] > 0;              // a set without a row that counts: sums 0, min / max NaN
        if (total) total[z] = wacc[2 * z];
        if (excluded) excluded[z] = wacc[2 * z + 1];
        for (size_t i = z * n; i < (z + 1) * n; i++) {
            if (s1) s1[i] = any ? acc[i].s1 : 0.0;
            if (s2) s2[i] = any ? acc[i].s2 : 0.0;
            if (vmin) vmin[i] = any ? acc[i].vmin : nan;
            if (vmax) vmax[i] = any ? acc[i].vmax : nan;
        }
    }
    return BH_OK;
}

extern "C" void bh_rf_sens_sets_destroy(void *handle)
{
    RfSensSets *s = (RfSensSets *)handle;
    if (!s) return;
    if (s->dedges) (void)hipStreamSynchronize(s->st);      // (a handle that never saw a row never saw the device)
    delete s;
}
