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
//   sens_sets_fold_kernel      (sens_sets_host.h, with nw = 1 weight pair a block) one thread per item, and one for the
//                              weights, adds the slab's rows to their sets' sums in block order.
//
// The slab holds a bounded number of blocks: a call's blocks are taken in chunks, each folded before the next is
// launched, which is the order of one pass over all of them.  The handle, that loop and the finish are
// sens_sets_host.h's SensSetsHandle; here are the main kernel, its arguments and launch, the samples, and the checks of
// what only this reduction takes.  create checks and records; the device is first touched by the first add that brings
// rows, after all of that call's arguments were checked.  No scratch; LDS rf_sens_sets_lds_doubles and the tile's sample
// offsets (14 464 B at 100 layers).
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

struct RfSensSets : bh::SensSetsHandle {          // nw = 1: a block carries one weight pair
    int nout = 0, nsel = 0;
    std::vector<int> samples;                      // [nsel]
    int *dsamples = nullptr;
};

// the first add that brings rows: the device, the samples, the handle's buffers
int make_ready(RfSensSets *s)
{
    if (s->ready) return BH_OK;
    if (int rc = bh::require_device()) return rc;
    BH_HIP(s->bufs.alloc(s->dsamples, (size_t)s->nsel));
    BH_HIP(hipMemcpyAsync(s->dsamples, s->samples.data(), sizeof(int) * s->nsel, hipMemcpyHostToDevice, s->st));
    return s->make_ready();
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
    s->init(set_start, nsets, edges, nedges, kind, drho_dvp, stream);
    s->nitems = (size_t)nsel * nedges;
    s->nout = nout;
    s->nsel = nsel;
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
    const char *own = !rf ? "NULL pointer"
                      : k_stride < (long long)s->nout * 4 * Lmax ? "k_stride < nout * 4 * Lmax"
                      : rf_stride < s->nout ? "rf_stride < nout" : nullptr;
    if (int rc = s->check_add(who, row0, B, Lmax, model_stride, nlay, hthk, q, q_stride, K, own)) return rc;
    if (B == 0) return BH_OK;
    if (int rc = make_ready(s)) return rc;
    RfSensSetsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.blocks = s->dblocks;
    a.Lmax = Lmax; a.mstride = model_stride; a.qstride = q_stride; a.rfstride = rf_stride; a.nsel = s->nsel; a.nb = s->nb;
    a.kind = s->kind; a.ctiles = bh::rf_sens_sets_cell_tiles(s->nb);
    a.kstride = k_stride;
    a.drho = s->drho;
    a.nlay = nlay; a.w = weights; a.samples = s->dsamples; a.h = hthk; a.q = q; a.K = K; a.rf = rf; a.edges = s->dedges;
    a.slab = s->slab; a.wslab = s->wslab; a.neg = s->neg;
    const unsigned tiles = (unsigned)(a.ctiles * bh::rf_sens_sets_sample_tiles(s->nsel));
    return s->add(who, row0, B, [&](unsigned nblocks) {
        hipLaunchKernelGGL(rf_sens_sets_kernel, dim3(nblocks, tiles), dim3(kThreads), lds_bytes(Lmax), s->st, a);
    });
}

extern "C" int bh_rf_sens_sets_finish(void *handle, long long *total, long long *excluded, double *s1, double *s2,
                                      double *vmin, double *vmax)
{
    const char *who = "bh_rf_sens_sets_finish";
    if (!handle) return bh::fail_who(who, "handle is NULL");
    return ((RfSensSets *)handle)->finish(who, total, excluded, s1, s2, vmin, vmax);
}

extern "C" void bh_rf_sens_sets_destroy(void *handle)
{
    delete (RfSensSets *)handle;
}
