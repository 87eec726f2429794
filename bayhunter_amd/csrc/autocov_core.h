// autocov_core.h -- the definition, the per-thread step and the LDS plan of the autocovariances of many run-length
// coded series (autocov.hip, bh_autocov_sets).
//
// A series is a run of rows, each repeated `weight` times: x_0 .. x_{n-1}, and y_t = x_t - mean (one rounded
// subtraction).  The result is defined exactly:
//
//     acov[k] = (acc_k after  acc_k = 0.0;  for t = 0 .. n-k-1 ascending: acc_k = fma(y_t, y_{t+k}, acc_k)) / (double)n
//
// one accumulator per (series, column, lag), 0 for k >= n and for n = 0.  Nothing in that chain depends on how the
// series is cut into tiles or how lags are dealt to threads: a tile only says when the accumulators rest, so the device
// returns the bits of the host build, whatever the grid.  (A NaN anywhere in y reaches every lag whose chain reads it.)
//
// A workgroup owns one (series, column, group of lags).  It expands and centres a tile of `tile` samples plus a halo of
// nlags samples into LDS, then every thread runs its kAutocovLags consecutive lags over the tile: y_t is one address
// for the whole wave, and because lag k + 1 at time t reads what lag k reads at t + 1 the thread keeps a window of
// y_{t+k ..} in registers and fetches ONE new sample per t for all its lags.  Thread i's window begins L samples after
// thread i - 1's, so the samples lie in LDS in L planes (sample m in plane m % L at m / L): the wave's fetch of a step
// is then 64 consecutive doubles of one plane instead of a stride of L doubles across the banks.
// Compiled with g++ under BH_HOSTSIM by tests/hostsim/autocov_sim.cpp (test infrastructure only).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/bayhunter_amd.h"      // BH_AUTOCOV_MAX_LAGS
#include "bh_common.h"

#if defined(BH_HOSTSIM)
#define BH_AUTOCOV_UNROLL
#else
#define BH_AUTOCOV_UNROLL _Pragma("unroll")
#endif

namespace bh {

constexpr int kAutocovLags = 8;                 // consecutive lags of a thread (L)
constexpr int kAutocovThreads = 256;            // threads of a workgroup at most: 2048 lags in a group
constexpr int kAutocovTile = 2048;              // samples of a tile (T)
constexpr int kAutocovLdsBytes = 64 * 1024;     // the most a workgroup asks for

// doubles of one plane for `tile` samples and a halo of nlags, L planes
BH_HD int autocov_pitch(int tile, int nlags, int L) { return (tile + nlags + L - 1) / L; }

// the LDS of a workgroup for nlags lags: the tile length and the bytes of its L planes (above kAutocovLdsBytes: refuse)
inline size_t autocov_plan(int nlags, int *tile)
{
    *tile = kAutocovTile;
    return sizeof(double) * (size_t)kAutocovLags * (size_t)autocov_pitch(kAutocovTile, nlags, kAutocovLags);
}

// lags of a group and threads of its workgroup (a multiple of 64) for nlags lags, L lags a thread
inline void autocov_groups(int nlags, int L, int max_threads, int *group_lags, int *threads)
{
    const int per = max_threads * L;
    *group_lags = nlags < per ? nlags : per;
    const int t = (*group_lags + L - 1) / L;
    *threads = (t + 63) / 64 * 64;
}

// where sample m of a tile lies among the L planes of `pitch` doubles
BH_HD int autocov_slot(int m, int L, int pitch) { return (m % L) * pitch + m / L; }

// the first row r of [ra, rb) whose expanded end cum(r + 1) lies above `pos`, rb when there is none.  cum[r] is the
// number of samples before row r (the exclusive prefix sum of the weights over all rows); NULL: every weight is 1
BH_HD long long autocov_first_row(const long long *cum, long long ra, long long rb, long long pos)
{
    if (!cum) return pos < ra ? ra : pos < rb ? pos : rb;
    long long lo = ra, hi = rb;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (cum[mid + 1] > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Row of value x spanning samples [a, a + w) of its series into the tile that holds samples [t0, t0 + len): its part
// of the tile, centred.  A row longer than a tile is met again by the next one.
BH_HD void autocov_expand_row(double *buf, int L, int pitch, long long t0, int len, long long a, long long w, double x,
                              double mean)
{
    const long long lo = a > t0 ? a : t0, hi = a + w < t0 + len ? a + w : t0 + len;
    const double y = x - mean;
    for (long long m = lo; m < hi; m++) buf[autocov_slot((int)(m - t0), L, pitch)] = y;
}

// A thread's step over one tile: lags k0 .. k0 + L - 1 (k0 a multiple of L), those below nlags, over the tile's `tl`
// times, of which lag k has n_left - k pairs left (n_left = n - t0: the samples from the tile's first to the series'
// end).  acc[j] goes on from the tile before.
template <int L>
BH_HD void autocov_tile(const double *buf, int pitch, int tl, long long n_left, int k0, int nlags, double *acc)
{
    int lim[L];
    BH_AUTOCOV_UNROLL
    for (int j = 0; j < L; j++) {
        const long long left = n_left - (k0 + j);
        lim[j] = k0 + j >= nlags || left <= 0 ? 0 : left < tl ? (int)left : tl;
    }
    const int all = lim[L - 1] / L * L;          // times at which every lag of the thread has a pair, in whole rounds
    const int q0 = k0 / L;
    if (all > 0) {
        double win[L];
        BH_AUTOCOV_UNROLL
        for (int j = 0; j < L - 1; j++) win[j] = buf[j * pitch + q0];
        for (int q = 0; q < all / L; q++) {
            BH_AUTOCOV_UNROLL
            for (int u = 0; u < L; u++) {
                // time i = q L + u: the window's new end y[i + k0 + L - 1] lies in plane (u + L - 1) % L
                win[(u + L - 1) % L] = buf[((u + L - 1) % L) * pitch + q + q0 + (u + L - 1) / L];
                const double yt = buf[u * pitch + q];
                BH_AUTOCOV_UNROLL
                for (int j = 0; j < L; j++) acc[j] = __builtin_fma(yt, win[(u + j) % L], acc[j]);
            }
        }
    }
    for (int i = all; i < lim[0]; i++) {         // the last times of a series' lags, and a thread's lags short of L
        const double yt = buf[autocov_slot(i, L, pitch)];
        BH_AUTOCOV_UNROLL
        for (int j = 0; j < L; j++)
            if (i < lim[j]) acc[j] = __builtin_fma(yt, buf[autocov_slot(i + k0 + j, L, pitch)], acc[j]);
    }
}

}  // namespace bh
