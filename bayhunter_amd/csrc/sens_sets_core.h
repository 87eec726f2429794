// sens_sets_core.h -- the per-row quantity and the order of the depth-binned sensitivity statistics (sens_sets.hip,
// bh_sens_sets_*): the layer kernel dc/dm of every sampled model spread over depth bins all models share, and its
// first two moments, minimum and maximum per set of rows, period and depth cell.
//
// A row r is a layered model (nlay, h[Lmax]) with what bh_sens_batch wrote for it (K[nper][4][Lmax], c_out[nper]), an
// optional ratio q[Lmax] (the layer's vp / vs) and an integer weight w.
//
//   layer value   G_l of period p (sens_sets_layer): K[1][l], K[2][l] or K[3][l] for BH_SENS_KIND_VP / _VS / _RHO;
//                 fma(q_l, fma(drho_dvp, K_rho, K_vp), K_vs) for BH_SENS_KIND_VS_TOTAL, the derivative with vp tied to
//                 vs and rho to vp (sensitivity.vs_total).  dc/dh is an interface derivative, not a depth density: not
//                 offered.
//   depth cells   with the edges e[0 .. nb] and the layer tops the sequential fp64 cumsum of h (sens_sets_tops), cell
//                 j < nb is x_j = sum over l = 0 .. nlay-2, ascending, by fma, of
//                 (max(0, min(bot_l, e[j+1]) - max(top_l, e[j])) / h_l) G_l; a layer with h_l <= 0 adds nothing, what
//                 lies outside e[0] .. e[nb] is dropped (sensitivity.to_depth).  Cell nb is the half-space's G_{nlay-1}.
//                 (sens_sets_cell; a term whose overlap is 0 is skipped, which changes no bit of a finite sum.)
//   who counts    (row, period) counts when w > 0, 2 <= nlay <= Lmax and c_out[p] is not NaN (sens_sets_counts):
//                 bh_sens_batch sets c_out, dc_dT and all of K of a (model, period) to NaN together.  A row with w > 0
//                 that does not count for a period adds w to the period's `excluded`.
//   the sums      per set, period and cell over the rows that count (SensSetsAcc): s1 = fma(w, x, s1), s2 = fma(fl(w x),
//                 x, s2), vmin, vmax; per set and period total = sum w.  No centre: DESIGN.md says why.
//
// The order (sens_sets_order).  A set's rows are cut into blocks of kSensSetsBlockRows rows, counted from the set's
// first row.  Inside a block the rows enter ascending, one chain per cell from (0, 0, +inf, -inf); the block partials
// are folded into the set's sums in ascending block order, s = s + partial from 0.0, by one thread per cell.  No
// floating-point atomic.  The rows may arrive in several calls that cut a set at block boundaries only: a set's result
// is a function of its rows alone -- not of the cuts, of its neighbours or of where its rows lie.
//
// A workgroup of kSensSetsThreads threads takes one block of rows and one group of kSensSetsThreads consecutive items,
// item = period * (nb + 1) + cell: one item per thread.  Per row it stages h, the tops, c_out and G of the periods its
// items touch in LDS (sens_sets_lds_doubles), then every thread walks the layers for its cell.
//
// Compiled with g++ under BH_HOSTSIM by tests/hostsim/sens_sets_sim.cpp (test infrastructure only).
#pragma once
#include "../../include/bayhunter_amd.h"      // BH_SENS_KIND_*, BH_SENS_SETS_BLOCK_ROWS, BH_SENS_SETS_MAX_BINS
#include "bh_common.h"

namespace bh {

constexpr int kSensSetsBlockRows = BH_SENS_SETS_BLOCK_ROWS;   // rows of a block: one partial per block and item
constexpr int kSensSetsThreads = 256;                         // items of a workgroup: one per thread

struct SensSetsAcc {
    double s1, s2, vmin, vmax;
};

BH_HD bool sens_sets_kind_ok(int kind) { return kind >= BH_SENS_KIND_VP && kind <= BH_SENS_KIND_VS_TOTAL; }

// periods the items of one workgroup can touch: kSensSetsThreads consecutive items of nb + 1 cells a period
BH_HD int sens_sets_span(int nper, int nb)
{
    const int s = (kSensSetsThreads - 1) / (nb + 1) + 2;
    return s < nper ? s : nper;
}

// doubles of a workgroup's LDS: h and the tops, then c_out and G[Lmax] per period of the span
BH_HD int sens_sets_lds_doubles(int Lmax, int nper, int nb) { return 2 * Lmax + sens_sets_span(nper, nb) * (Lmax + 1); }

BH_HD bool sens_sets_counts(int w, int nlay, int Lmax, double c) { return w > 0 && nlay >= 2 && nlay <= Lmax && c == c; }

// G_l of one period: K the period's [4][Lmax] block, q the row's ratios (BH_SENS_KIND_VS_TOTAL only)
BH_HD double sens_sets_layer(int kind, double drho_dvp, const double *K, int Lmax, const double *q, int l)
{
    if (kind == BH_SENS_KIND_VS_TOTAL)
        return __builtin_fma(q[l], __builtin_fma(drho_dvp, K[3 * Lmax + l], K[Lmax + l]), K[2 * Lmax + l]);
    return K[kind * Lmax + l];
}

// tops[0 .. nlay-1] from h[0 .. nlay-2]: tops[nlay - 1] is the top of the half-space
BH_HD void sens_sets_tops(const double *h, int nlay, double *tops)
{
    double t = 0.0;
    for (int l = 0; l < nlay - 1; l++) {
        tops[l] = t;
        t = t + h[l];
    }
    tops[nlay - 1] = t;
}

// cell j of one period: G the period's layer values
BH_HD double sens_sets_cell(const double *tops, const double *h, const double *G, int nlay, const double *edges, int nb,
                            int j)
{
    if (j == nb) return G[nlay - 1];
    const double e0 = edges[j], e1 = edges[j + 1];
    double x = 0.0;
    for (int l = 0; l < nlay - 1; l++) {
        const double top = tops[l], bot = tops[l + 1];
        const double lo = top > e0 ? top : e0, hi = bot < e1 ? bot : e1;
        const double d = hi - lo;
        if (d > 0.0 && h[l] > 0.0) x = __builtin_fma(d / h[l], G[l], x);
    }
    return x;
}

BH_HD void sens_sets_acc_init(SensSetsAcc &a)
{
    a.s1 = 0.0;
    a.s2 = 0.0;
    a.vmin = __builtin_inf();
    a.vmax = -__builtin_inf();
}

// a row that counts enters its block's chain
BH_HD void sens_sets_acc_row(SensSetsAcc &a, double w, double x)
{
    a.s1 = __builtin_fma(w, x, a.s1);
    const double wx = w * x;
    a.s2 = __builtin_fma(wx, x, a.s2);
    a.vmin = x < a.vmin ? x : a.vmin;
    a.vmax = x > a.vmax ? x : a.vmax;
}

// a block's partial enters its set's sums
BH_HD void sens_sets_acc_fold(SensSetsAcc &a, const SensSetsAcc &p)
{
    a.s1 = a.s1 + p.s1;
    a.s2 = a.s2 + p.s2;
    a.vmin = p.vmin < a.vmin ? p.vmin : a.vmin;
    a.vmax = p.vmax > a.vmax ? p.vmax : a.vmax;
}

}  // namespace bh
