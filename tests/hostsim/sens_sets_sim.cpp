// sens_sets_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the core of the depth-binned sensitivity statistics (bayhunter_amd/csrc/sens_sets_core.h) with g++ and
// replays what sens_sets.hip does with it on the host: per set the blocks of kSensSetsBlockRows rows from the set's first
// row, in a block the rows ascending through the same layer value, tops, cell walk and chain, the block partials
// folded in block order.  The CPU tier holds it against the longdouble restatement (tests/sens_sets_ref.py), the GPU
// tier holds the kernels against it bit for bit.
#define BH_HOSTSIM 1
#include <cmath>
#include <vector>
#include "../../bayhunter_amd/csrc/sens_sets_core.h"

// rows 0 .. R-1 in sets start[0 .. nsets]; outputs as bh_sens_sets_finish writes them.  -> 1 for a negative weight
extern "C" int sss_sets(const long long *start, int nsets, int nper, const double *edges, int nedges, int kind,
                        double drho, int Lmax, int mstride, const int *nlay, const double *h, const double *q, int qstride,
                        const double *K, const double *c, const int *w, long long *total, long long *excluded, double *s1,
                        double *s2, double *vmin, double *vmax)
{
    const int nb = nedges - 1, cells = nb + 1;
    const size_t nitems = (size_t)nper * cells;
    for (long long r = 0; r < start[nsets]; r++)
        if (w && w[r] < 0) return 1;
    std::vector<double> tops(Lmax), G(Lmax);
    std::vector<bh::SensSetsAcc> acc(nitems), part(nitems);
    for (int z = 0; z < nsets; z++) {
        for (auto &a : acc) bh::sens_sets_acc_init(a);
        long long *tot = total + (size_t)z * nper, *exc = excluded + (size_t)z * nper;
        for (int p = 0; p < nper; p++) tot[p] = exc[p] = 0;
        for (long long b0 = start[z]; b0 < start[z + 1]; b0 += bh::kSensSetsBlockRows) {
            const long long b1 = b0 + bh::kSensSetsBlockRows < start[z + 1] ? b0 + bh::kSensSetsBlockRows : start[z + 1];
            for (auto &a : part) bh::sens_sets_acc_init(a);
            for (long long r = b0; r < b1; r++) {
                const int wr = w ? w[r] : 1, nl = nlay[r];
                if (wr <= 0) continue;
                const bool model = nl >= 2 && nl <= Lmax;
                if (model) bh::sens_sets_tops(h + r * mstride, nl, tops.data());
                for (int p = 0; p < nper; p++) {
                    if (!model || !bh::sens_sets_counts(wr, nl, Lmax, c[r * nper + p])) {
                        exc[p] += wr;
                        continue;
                    }
                    tot[p] += wr;
                    for (int l = 0; l < nl; l++)
                        G[l] = bh::sens_sets_layer(kind, drho, K + (r * nper + p) * 4 * Lmax, Lmax, q ? q + r * qstride : nullptr, l);
                    for (int j = 0; j < cells; j++)
                        bh::sens_sets_acc_row(part[(size_t)p * cells + j], (double)wr,
                                              bh::sens_sets_cell(tops.data(), h + r * mstride, G.data(), nl, edges, nb, j));
                }
            }
            for (size_t i = 0; i < nitems; i++) bh::sens_sets_acc_fold(acc[i], part[i]);
        }
        for (int p = 0; p < nper; p++)
            for (int j = 0; j < cells; j++) {
                const size_t i = (size_t)p * cells + j, o = (size_t)z * nitems + i;
                const bool any = tot[p] > 0;
                s1[o] = any ? acc[i].s1 : 0.0;
                s2[o] = any ? acc[i].s2 : 0.0;
                vmin[o] = any ? acc[i].vmin : std::nan("");
                vmax[o] = any ? acc[i].vmax : std::nan("");
            }
    }
    return 0;
}

extern "C" int sss_block_rows(void) { return bh::kSensSetsBlockRows; }
extern "C" int sss_threads(void) { return bh::kSensSetsThreads; }
extern "C" int sss_lds_bytes(int Lmax, int nper, int nb) { return 8 * bh::sens_sets_lds_doubles(Lmax, nper, nb); }
