// rf_sens_sets_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the core of the depth-binned receiver-function sensitivity statistics (bayhunter_amd/csrc/rf_sens_sets_core.h,
// on top of sens_sets_core.h) with g++ and replays what rf_sens_sets.hip does with it on the host: per set the blocks of
// kSensSetsBlockRows rows from the set's first row, in a block the rows ascending; per row the tops, and per group of
// kRfSensSetsRS selected samples the layer values G[l][sample] and, for every cell, the blocked walk rf_sens_sets_cells
// and the chains rf_sens_sets_acc_rows -- what one thread of the kernel does --; the block partials folded in block
// order.  The CPU tier holds it against the longdouble restatement (tests/rf_sens_sets_ref.py) and against
// sens_sets_sim.cpp, the GPU tier holds the kernels against it bit for bit.
#define BH_HOSTSIM 1
#include <cmath>
#include <vector>
#include "../../bayhunter_amd/csrc/rf_sens_sets_core.h"

// rows 0 .. R-1 in sets start[0 .. nsets]; samples [nsel] or NULL for all nout; outputs as bh_rf_sens_sets_finish writes
// them.  -> 1 for a negative weight
extern "C" int rss_sets(const long long *start, int nsets, int nout, const int *samples, int nsel, const double *edges,
                        int nedges, int kind, double drho, int Lmax, int mstride, const int *nlay, const double *h,
                        const double *q, int qstride, const double *K, long long kstride, const double *rf, int rfstride,
                        const int *w, long long *total, long long *excluded, double *s1, double *s2, double *vmin,
                        double *vmax)
{
    constexpr int RS = bh::kRfSensSetsRS, TS = bh::kRfSensSetsTileSamples;
    if (!samples) nsel = nout;
    const int nb = nedges - 1, cells = nb + 1;
    const size_t nitems = (size_t)nsel * cells;
    for (long long r = 0; r < start[nsets]; r++)
        if (w && w[r] < 0) return 1;
    std::vector<double> tops(Lmax), G((size_t)Lmax * TS);
    std::vector<bh::SensSetsAcc> acc(nitems), part(nitems);
    for (int z = 0; z < nsets; z++) {
        for (auto &a : acc) bh::sens_sets_acc_init(a);
        long long tot = 0, exc = 0;
        for (long long b0 = start[z]; b0 < start[z + 1]; b0 += bh::kSensSetsBlockRows) {
            const long long b1 = b0 + bh::kSensSetsBlockRows < start[z + 1] ? b0 + bh::kSensSetsBlockRows : start[z + 1];
            for (auto &a : part) bh::sens_sets_acc_init(a);
            for (long long r = b0; r < b1; r++) {
                const int wr = w ? w[r] : 1, nl = nlay[r];
                if (wr <= 0) continue;
                if (!bh::rf_sens_sets_counts(wr, nl, Lmax, nl >= 2 && nl <= Lmax ? rf[r * rfstride] : 0.0)) {
                    exc += wr;
                    continue;
                }
                tot += wr;
                const double *hrow = h + r * mstride, *qrow = q ? q + r * qstride : nullptr, *Krow = K + r * kstride;
                bh::sens_sets_tops(hrow, nl, tops.data());
                for (int t0 = 0; t0 < nsel; t0 += TS) {                         // a tile's samples
                    const int nt = nsel - t0 < TS ? nsel - t0 : TS;
                    for (auto &g : G) g = 0.0;
                    for (int s = 0; s < nt; s++)
                        for (int l = 0; l < nl; l++)
                            G[(size_t)l * TS + s] = bh::sens_sets_layer(
                                kind, drho, Krow + (size_t)(samples ? samples[t0 + s] : t0 + s) * 4 * Lmax, Lmax, qrow, l);
                    for (int s0 = 0; s0 < nt; s0 += RS)                         // a thread: one cell, RS samples
                        for (int j = 0; j < cells; j++) {
                            double x[RS];
                            bh::SensSetsAcc a[RS];
                            for (int s = 0; s < RS; s++)
                                if (s0 + s < nt) a[s] = part[(size_t)(t0 + s0 + s) * cells + j];
                                else bh::sens_sets_acc_init(a[s]);
                            bh::rf_sens_sets_cells<RS>(tops.data(), hrow, G.data() + s0, TS, nl, j < nb ? edges[j] : 0.0,
                                                       j < nb ? edges[j + 1] : 0.0, j == nb, x);
                            bh::rf_sens_sets_acc_rows<RS>(a, (double)wr, x);
                            for (int s = 0; s < RS && s0 + s < nt; s++) part[(size_t)(t0 + s0 + s) * cells + j] = a[s];
                        }
                }
            }
            for (size_t i = 0; i < nitems; i++) bh::sens_sets_acc_fold(acc[i], part[i]);
        }
        total[z] = tot;
        excluded[z] = exc;
        const bool any = tot > 0;
        for (size_t i = 0; i < nitems; i++) {
            const size_t o = (size_t)z * nitems + i;
            s1[o] = any ? acc[i].s1 : 0.0;
            s2[o] = any ? acc[i].s2 : 0.0;
            vmin[o] = any ? acc[i].vmin : std::nan("");
            vmax[o] = any ? acc[i].vmax : std::nan("");
        }
    }
    return 0;
}

extern "C" int rss_rs(void) { return bh::kRfSensSetsRS; }
extern "C" int rss_tile_cells(void) { return bh::kRfSensSetsCells; }
extern "C" int rss_tile_samples(void) { return bh::kRfSensSetsTileSamples; }
extern "C" int rss_threads(void) { return bh::kRfSensSetsThreads; }
extern "C" int rss_lds_bytes(int Lmax) { return 8 * bh::rf_sens_sets_lds_doubles(Lmax) + 4 * bh::kRfSensSetsTileSamples; }
