// datacov_core.h -- the definition, the blocking and the per-row steps of the cross moment of Vs(z) and the modelled
// data (datacov.hip, bh_datacov_sets).
//
// A row r of a set has K = ndep + nextra model columns -- x_rk, exactly the columns of depthcov_core.h: its Vs on the
// depth grid (PostWalk) followed by its `extra` values -- and S data columns y_rj = Y[r][col0 + j].  A row COUNTS when
// its weight w_r > 0, it has a model (post_row_count >= 2), all its err flags are 0 and none of its S data values is
// NaN: the rows bh_datafits keeps.  That is decided once per row from all S columns (datacov_effective, the pre-pass)
// and handed on as the row's effective weight, so that every workgroup, whichever data columns it holds, takes the same
// rows.  Every other row is a row of zeros: it changes no bit.  With cx [K] and cy [S] the set's centres, any centres,
//
//     dx_rk = fl(x_rk - cx_k)      ex_rk = fl((double)w_r dx_rk)
//     dy_rj = fl(y_rj - cy_j)      ey_rj = fl((double)w_r dy_rj)
//     C_kj  = sum_r ex_rk dy_rj                               [K][S]
//     r1x_k = sum_r ex_rk          r1y_j = sum_r ey_rj
//     qx_k  = sum_r ex_rk dx_rk    qy_j  = sum_r ey_rj dy_rj
//     total = sum_r w_r            excluded = sum of w_r over the rows with w_r > 0 that do not count
//
// The order of the sums is depthcov's.  A set's rows are cut into blocks of kDepthcovBlockRows rows, counted from the
// set's first row.  Inside a block the rows enter in ascending order: C on the device four at a time, one
// v_mfma_f64_16x16x4_f64 per 16 x 16 tile and four rows, the accumulator zero at the block's first row; in the host
// twin (tests/hostsim/datacov_sim.cpp) acc = fma(ex_rk, dy_rj, acc) row by row.  qx and qy are the chains
// acc = fma(e, d, acc) and r1x, r1y the plain sums acc = acc + e in the same order, on both sides.  The block partials
// are then added in ascending block order, from 0.0, by one thread per cell (datacov_fold_kernel): no atomics on
// floating point.  So a set's result is a function of the set's rows, centres and grid alone; and a cell of column j
// is a function of column j and of WHICH rows count, not of the other data columns' values.
//
// Tiles.  K is padded to Kp = 16 Tx and S to Sp = 16 Ty; all Tx x Ty tile pairs are computed (no triangle), pair
// p = tj Tx + ti.  The data-column tiles are dealt to workgroups in groups of G = datacov_group_tiles(Tx) tiles, so
// that a group's Tx G pairs fit the workgroup's kDepthcovGroupPairs accumulators: a workgroup's LDS holds all Kp model
// columns and the 16 G data columns of its own group.
//
// Compiled with g++ under BH_HOSTSIM by tests/hostsim/datacov_sim.cpp (test infrastructure only).
#pragma once
#include "depthcov_core.h"

namespace bh {

constexpr int kDatacovMaxGroupTiles = 16;       // data-column tiles of a group at most: 256 columns, a thread each

BH_HD constexpr int datacov_group_tiles(int Tx)
{
    return kDepthcovGroupPairs / Tx < kDatacovMaxGroupTiles ? kDepthcovGroupPairs / Tx : kDatacovMaxGroupTiles;
}
// doubles between two rows of a stage, as depthcov_pitch: the four rows of a k-step start 32 banks apart
BH_HD constexpr int datacov_pitch(int cols) { return depthcov_pitch(cols); }
// the LDS of a workgroup in doubles: two stages of ex [SR][pitch(Kp)] and of dy [SR][pitch(Yc)], one stage of dx (the
// factor qx needs beside ex), the grid, cx and the group's cy
BH_HD constexpr int datacov_lds_doubles(int Kp, int Yc)
{
    return kDepthcovStageRows * (3 * datacov_pitch(Kp) + 2 * datacov_pitch(Yc)) + 2 * Kp + Yc;
}
// the widest: over every Tx with its own group width
BH_HD constexpr int datacov_max_lds_doubles()
{
    int most = 0;
    for (int Tx = 1; Tx <= BH_DEPTHCOV_MAX_K / 16; Tx++) {
        const int n = datacov_lds_doubles(16 * Tx, 16 * datacov_group_tiles(Tx));
        most = n > most ? n : most;
    }
    return most;
}

// The effective weight of a row, decided once from all S data columns: w when the row counts, -w when it has w > 0 and
// does not count (its weight goes to `excluded`), 0 for w = 0.  w >= 0 (a negative weight is the caller's error).
// `y` the row's S data values, `err` its nflags flags (NULL: none).
template <typename T>
BH_HD int datacov_effective(const T *row, int width, int w, const double *y, int S, const int *err, int nflags)
{
    if (w <= 0) return 0;
    bool ok = post_row_count(row, width) >= 2;
    for (int f = 0; ok && f < nflags; f++) ok = err[f] == 0;
    for (int j = 0; ok && j < S; j++) ok = y[j] == y[j];
    return ok ? w : -w;
}

// Model columns c0, c0 + step, .. below c1 of one row into its stage row: ex[c] and, where dx is not NULL, dx[c]; zeros
// beyond K and for a row that does not count (weff <= 0; `row` may then be NULL).  depthcov_row's walk and arithmetic.
template <typename T>
BH_HD void datacov_row_x(const T *row, int width, int weff, const double *extra, int ndep, int nextra, const double *dep,
                         const double *cx, int c0, int c1, int step, double *ex, double *dx)
{
    const int K = ndep + nextra;
    const bool in = weff > 0;
    const double dw = (double)weff;
    PostWalk<T> wk;
    wk.init(row, in ? post_row_count(row, width) : 0);
    for (int c = c0; c < c1; c += step) {
        double v = 0.0, wv = 0.0;
        if (in && c < K) {
            const double x = c < ndep ? (double)wk.at(dep[c]) : extra[c - ndep];
            v = x - cx[c];
            wv = dw * v;
        }
        ex[c] = wv;
        if (dx) dx[c] = v;
    }
}

// Data columns j0 + c0, j0 + c0 + step, .. below j0 + c1 of one row into dy[c0 ..]: zeros beyond S and for a row that
// does not count.  `y` the row's S data values, cy the centres from column j0 on (cy[c] is column j0 + c's).
BH_HD void datacov_row_y(const double *y, int weff, int S, const double *cy, int j0, int c0, int c1, int step, double *dy)
{
    for (int c = c0; c < c1; c += step) {
        const int j = j0 + c;
        dy[c] = (weff > 0 && j < S) ? y[j] - cy[c] : 0.0;
    }
}

}  // namespace bh
