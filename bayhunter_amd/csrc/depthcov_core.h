// depthcov_core.h -- the definition, the blocking and the per-row step of the depth-to-depth second moment of Vs
// (depthcov.hip, bh_depthcov_sets).
//
// A row r of a set has K = ndep + nextra columns: x_rk its Vs on the depth grid (PostWalk, posterior_core.h) followed by
// its `extra` values.  With c the set's centre and w_r the row's integer weight
//
//     d_rk = fl(x_rk - c_k)        one rounded subtraction
//     e_rk = fl((double)w_r d_rk)  one rounded product
//     S_ij = sum_r e_ri d_rj,   r1_i = sum_r e_ri,   total = sum_r w_r      over the rows with w_r > 0 and a model
//
// (a model: at least one nucleus, post_row_count >= 2).  A row left out is a row of zeros: it changes no bit.
//
// The order of the sums is fixed.  A set's rows are cut into blocks of kDepthcovBlockRows rows, counted from the set's
// first row.  Inside a block the rows enter in ascending order: on the device four at a time, one
// v_mfma_f64_16x16x4_f64 per 16 x 16 tile of S and four rows, the accumulator zero at the block's first row; in the host
// twin (tests/hostsim/depthcov_sim.cpp) acc = fma(e_ri, d_rj, acc) row by row.  r1 is the plain sum acc = acc + e_ri in
// the same order, on both sides.  The block partials are then added in ascending block order, from 0.0, by one thread per
// cell (depthcov_fold_kernel): no atomics.  So a set's result is a function of the set's rows, centre and grid alone:
// two runs agree bit for bit, and neither the other sets of a call nor the set's offset in `rows` change a bit.
//
// Tiles.  K is padded to Kp = 16 T; only the tile pairs (i, j) with j >= i are computed, pair p = 0 .. T (T + 1) / 2 - 1
// in row-major order of the upper triangle (depthcov_pair).  An off-diagonal tile (i, j) gives S[16 i + m][16 j + n]
// and, mirrored, S[16 j + n][16 i + m].  A DIAGONAL tile (i, i) holds both orders of every off-diagonal cell, which
// differ in which factor carries the rounded weight: its cells with n >= m are taken and mirrored, the others are
// dropped.  S is therefore exactly symmetric, and S[a][b] for a <= b is always sum_r e_ra d_rb.
//
// Compiled with g++ under BH_HOSTSIM by tests/hostsim/depthcov_sim.cpp (test infrastructure only).
#pragma once
#include "../../include/bayhunter_amd.h"      // BH_DEPTHCOV_MAX_K, BH_DEPTHCOV_BLOCK_ROWS
#include "bh_common.h"
#include "posterior_core.h"

namespace bh {

constexpr int kDepthcovBlockRows = BH_DEPTHCOV_BLOCK_ROWS;   // rows of a block (B): one partial of S per block
constexpr int kDepthcovStageRows = 16;          // rows a workgroup walks into LDS at a time (four MFMA k-steps)
constexpr int kDepthcovWaves = 8;               // waves of a workgroup: two per SIMD
constexpr int kDepthcovThreads = 64 * kDepthcovWaves;
constexpr int kDepthcovWavePairs = 12;          // tile pairs (accumulators of 4 doubles a lane) a wave holds
constexpr int kDepthcovGroupPairs = kDepthcovWaves * kDepthcovWavePairs;   // of a workgroup: 96 >= the 91 of 201 depths
constexpr int kDepthcovTile = 256;              // doubles of a tile partial in the slab, in the accumulator's order

static_assert(kDepthcovBlockRows % kDepthcovStageRows == 0 && kDepthcovStageRows % 4 == 0, "whole stages, whole k-steps");
static_assert(kDepthcovThreads % kDepthcovStageRows == 0, "the same number of threads walks every row of a stage");

BH_HD constexpr int depthcov_kp(int K) { return (K + 15) / 16 * 16; }
// doubles between two rows of a stage: Kp, and 16 more when Kp is a multiple of 32, so that the four rows of a k-step
// start 32 banks apart and a wave's 4 x 16 doubles cover the 64 banks once
BH_HD constexpr int depthcov_pitch(int Kp) { return Kp % 32 ? Kp : Kp + 16; }
BH_HD constexpr int depthcov_npairs(int T) { return T * (T + 1) / 2; }
BH_HD long long depthcov_blocks(long long rows) { return (rows + kDepthcovBlockRows - 1) / kDepthcovBlockRows; }
// the LDS of a workgroup: two stages of d and e, the grid and the centre
BH_HD constexpr int depthcov_lds_doubles(int Kp) { return 4 * kDepthcovStageRows * depthcov_pitch(Kp) + 2 * Kp; }

// pair p of the upper triangle of T x T tiles, row-major: (0,0) (0,1) .. (0,T-1) (1,1) ..
BH_HD void depthcov_pair(int T, int p, int *i, int *j)
{
    int a = 0;
    while (p >= T - a) {
        p -= T - a;
        a++;
    }
    *i = a;
    *j = a + p;
}

// where cell (m, n) of a tile lies in the accumulator of v_mfma_f64_16x16x4_f64, as reg * 64 + lane: the column on the
// lane's low four bits, row = (lane >> 4) + 4 reg
BH_HD int depthcov_acc_slot(int m, int n) { return (m >> 2) * 64 + (m & 3) * 16 + n; }

// Columns c0, c0 + step, .. below c1 of one row into its stage row: d[c] and e[c], zeros beyond K and for a row left
// out.  `row` may be NULL (a slot past the set's end).  dep [ndep] ascending, center [K], extra the row's nextra values.
// Every caller walks the row from its top: the columns of a row may be dealt to any number of threads.  -> the row counts
template <typename T>
BH_HD bool depthcov_row(const T *row, int width, int w, const double *extra, int ndep, int nextra, const double *dep,
                        const double *center, int c0, int c1, int step, double *d, double *e)
{
    const int K = ndep + nextra;
    const int count = row ? post_row_count(row, width) : 0;
    const bool in = w > 0 && count >= 2;
    const double dw = (double)w;
    PostWalk<T> wk;
    wk.init(row, in ? count : 0);
    for (int c = c0; c < c1; c += step) {
        double v = 0.0, wv = 0.0;
        if (in && c < K) {
            const double x = c < ndep ? (double)wk.at(dep[c]) : extra[c - ndep];
            v = x - center[c];
            wv = dw * v;
        }
        d[c] = v;
        e[c] = wv;
    }
    return in;
}

}  // namespace bh
