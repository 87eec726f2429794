// rf_sens_sets_core.h -- the per-thread body of the depth-binned receiver-function sensitivity statistics
// (rf_sens_sets.hip, bh_rf_sens_sets_*): dRF(t)/dm of every sampled model spread over depth bins all models share, and
// its first two moments, minimum and maximum per set of rows, selected sample of the trace and depth cell.
//
// The quantity and the order of the sums are those of sens_sets_core.h, with a trace's samples where that file has
// periods: the layer value is sens_sets_layer on the sample's [4][Lmax] block of K, the tops are sens_sets_tops, cell j of
// a sample is sens_sets_cell's chain, a row enters by sens_sets_acc_row and a block partial by sens_sets_acc_fold, in
// blocks of kSensSetsBlockRows rows from the set's first row.  What differs is who counts and how the work is cut:
//
//   who counts    a row counts for all samples or for none: w > 0, 2 <= nlay <= Lmax and rf[0] is not NaN (bh_rf_batch
//                 gives NaN throughout for a model without a trace).  total and excluded are per set.
//   the tile      a workgroup of kRfSensSetsThreads threads takes one block of rows, kRfSensSetsCells consecutive depth
//                 cells and kRfSensSetsTileSamples consecutive selected samples.  Thread tid owns cell tid %
//                 kRfSensSetsCells and the kRfSensSetsRS samples of group tid / kRfSensSetsCells: the lanes of a wave
//                 share their samples and differ in the cell, so a wave reads G[l][sample] as one broadcast.
//   the walk      the overlap of layer l with bin j depends on the row and the bin only.  A thread walks the row's
//                 layers once, forms d / h_l once per layer that overlaps its bin and applies it to its RS chains
//                 (rf_sens_sets_cells): per chain the operations of sens_sets_cell, in its order, so that every cell has
//                 sens_sets_cell's bits.
//
// Compiled with g++ under BH_HOSTSIM by tests/hostsim/rf_sens_sets_sim.cpp (test infrastructure only).
#pragma once
#include "sens_sets_core.h"

namespace bh {

constexpr int kRfSensSetsThreads = 256;
constexpr int kRfSensSetsRS = 4;                                                  // samples a thread blocks in registers
constexpr int kRfSensSetsCells = 64;                                              // cells of a tile: one wave wide
constexpr int kRfSensSetsGroups = kRfSensSetsThreads / kRfSensSetsCells;          // sample groups of a tile
constexpr int kRfSensSetsTileSamples = kRfSensSetsGroups * kRfSensSetsRS;         // samples of a tile

// doubles of a workgroup's LDS: h and the tops, then G[Lmax][kRfSensSetsTileSamples]
BH_HD int rf_sens_sets_lds_doubles(int Lmax) { return (2 + kRfSensSetsTileSamples) * Lmax; }

BH_HD int rf_sens_sets_cell_tiles(int nb) { return (nb + 1 + kRfSensSetsCells - 1) / kRfSensSetsCells; }
BH_HD int rf_sens_sets_sample_tiles(int nsel) { return (nsel + kRfSensSetsTileSamples - 1) / kRfSensSetsTileSamples; }

// rf0 the first sample of the row's trace
BH_HD bool rf_sens_sets_counts(int w, int nlay, int Lmax, double rf0) { return sens_sets_counts(w, nlay, Lmax, rf0); }

// Cell j of RS samples at once: G the layer values of the group's first sample at layer 0, laid out [l][lstride] with the
// samples of a layer side by side, so that a thread reads its RS values of a layer as one stretch; e0, e1 the bin's edges
// (j < nb), half: j == nb, the half-space.  x[s] is sens_sets_cell's value for sample s: its operations, in its order.
template <int RS>
BH_HD void rf_sens_sets_cells(const double *tops, const double *h, const double *G, int lstride, int nlay, double e0,
                              double e1, bool half, double (&x)[RS])
{
    if (half) {
#pragma unroll
        for (int s = 0; s < RS; s++) x[s] = G[(nlay - 1) * lstride + s];
        return;
    }
#pragma unroll
    for (int s = 0; s < RS; s++) x[s] = 0.0;
#pragma unroll 1
    for (int l = 0; l < nlay - 1; l++) {          // (one trip at a time: an unrolled walk holds several trips' G in registers)
        const double top = tops[l], bot = tops[l + 1];
        const double lo = top > e0 ? top : e0, hi = bot < e1 ? bot : e1;
        const double d = hi - lo;
        if (d > 0.0 && h[l] > 0.0) {
            const double f = d / h[l];
#pragma unroll
            for (int s = 0; s < RS; s++) x[s] = __builtin_fma(f, G[l * lstride + s], x[s]);
        }
    }
}

// a row that counts enters the chains of a thread's RS samples
template <int RS>
BH_HD void rf_sens_sets_acc_rows(SensSetsAcc (&acc)[RS], double w, const double (&x)[RS])
{
#pragma unroll
    for (int s = 0; s < RS; s++) sens_sets_acc_row(acc[s], w, x[s]);
}

}  // namespace bh
