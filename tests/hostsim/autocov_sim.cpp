// autocov_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the core of the autocovariances (bayhunter_amd/csrc/autocov_core.h) with g++ so that the CPU tier replays
// the kernel's walk -- the prefix sum of the weights, a block per (series, column, group of lags), tiles with their
// halo expanded row by row into the planes, every thread's step over a tile -- against the numpy restatement
// (tests/convergence_ref.py), under the library's tile length and lag grouping and under others.
// With AUTOCOV_SIM_MAIN a stand-alone program over built shapes for a sanitizer build (tests/test_convergence.py).
#define BH_HOSTSIM 1
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/autocov_core.h"

namespace {

template <int L>
void walk(const double *D, long long stride, int ncols, const long long *cum, const long long *start, int nseries,
          const double *mean, int nlags, double *acov, int tile, int max_threads)
{
    int group_lags = 0, threads = 0;
    bh::autocov_groups(nlags, L, max_threads, &group_lags, &threads);
    const int ngroups = (nlags + group_lags - 1) / group_lags;
    const int pitch = bh::autocov_pitch(tile, nlags, L);
    std::vector<double> buf((size_t)L * pitch), acc((size_t)threads * L);
    for (int s = 0; s < nseries; s++)
        for (int c = 0; c < ncols; c++)
            for (int g = 0; g < ngroups; g++) {
                const long long ra = start[s], rb = start[s + 1];
                const long long base = cum ? cum[ra] : ra;
                const long long n = (cum ? cum[rb] : rb) - base;
                std::fill(acc.begin(), acc.end(), 0.0);
                for (long long t0 = 0; t0 < n; t0 += tile) {
                    const long long left = n - t0;
                    const int tl = left < tile ? (int)left : tile;
                    const int len = left < tile + nlags ? (int)left : tile + nlags;
                    std::fill(buf.begin(), buf.end(), std::nan(""));       // what no row wrote must not be read
                    const long long first = bh::autocov_first_row(cum, ra, rb, base + t0);
                    for (int tid = 0; tid < threads; tid++)
                        for (long long r = first + tid; r < rb; r += threads) {
                            const long long at = (cum ? cum[r] : r) - base;
                            if (at >= t0 + len) break;
                            const long long w = cum ? cum[r + 1] - cum[r] : 1;
                            if (w > 0)
                                bh::autocov_expand_row(buf.data(), L, pitch, t0, len, at, w, D[r * stride + c],
                                                       mean[(size_t)s * ncols + c]);
                        }
                    for (int tid = 0; tid < threads; tid++)
                        bh::autocov_tile<L>(buf.data(), pitch, tl, left, g * group_lags + tid * L, nlags, &acc[(size_t)tid * L]);
                }
                double *out = acov + ((size_t)s * ncols + c) * nlags;
                for (int tid = 0; tid < threads; tid++)
                    for (int j = 0; j < L; j++) {
                        const int k = g * group_lags + tid * L + j;
                        if (k < nlags && k < (g + 1) * group_lags) out[k] = n > 0 ? acc[(size_t)tid * L + j] / (double)n : 0.0;
                    }
            }
}

}  // namespace

// the dynamic LDS bytes of a workgroup and its tile length, as the library plans them
extern "C" long as_plan(int nlags, int *tile) { return (long)bh::autocov_plan(nlags, tile); }
extern "C" int as_lags_per_thread(void) { return bh::kAutocovLags; }

// bh_autocov_sets as its kernels walk it.  tile, lags_per_thread (1, 2, 4 or 8) and max_threads (a multiple of 64): 0
// for the library's.  -> 0, 1 for a negative weight, 2 for a shape the walk does not take
extern "C" int as_autocov_sets(const double *D, long long nrows, long long stride, int ncols, const int *weights,
                               const long long *series_start, int nseries, const double *mean, int nlags, double *acov,
                               long long *length, int tile, int lags_per_thread, int max_threads)
{
    std::vector<long long> cum;
    if (weights) {
        cum.assign((size_t)nrows + 1, 0);
        for (long long r = 0; r < nrows; r++) {
            if (weights[r] < 0) return 1;
            cum[r + 1] = cum[r] + weights[r];
        }
    }
    const long long *pc = weights ? cum.data() : nullptr;
    for (int s = 0; s < nseries; s++)
        length[s] = pc ? pc[series_start[s + 1]] - pc[series_start[s]] : series_start[s + 1] - series_start[s];
    if (tile < 1) bh::autocov_plan(nlags, &tile);
    if (max_threads < 1) max_threads = bh::kAutocovThreads;
    if (max_threads % 64) return 2;
    switch (lags_per_thread ? lags_per_thread : bh::kAutocovLags) {
    case 1: walk<1>(D, stride, ncols, pc, series_start, nseries, mean, nlags, acov, tile, max_threads); break;
    case 2: walk<2>(D, stride, ncols, pc, series_start, nseries, mean, nlags, acov, tile, max_threads); break;
    case 4: walk<4>(D, stride, ncols, pc, series_start, nseries, mean, nlags, acov, tile, max_threads); break;
    case 8: walk<8>(D, stride, ncols, pc, series_start, nseries, mean, nlags, acov, tile, max_threads); break;
    default: return 2;
    }
    return 0;
}

#if defined(AUTOCOV_SIM_MAIN)
// The CPU tier's shapes through the walk, for a build with -fsanitize=address,undefined: expanded lengths around the
// tile, every nlags of the tests, weights 0 .. 5, one row longer than three tiles, a stride wider than the columns;
// each against the definition's plain loop.  Prints the number of results compared; exit status 1 on a difference.
static unsigned long long g_seed = 88172645463325252ull;
static double rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (double)(g_seed >> 11) / 9007199254740992.0;
}

int main()
{
    int T = 0;
    bh::autocov_plan(64, &T);
    const long long lens[] = {0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, T + 64 + 1, 3 * T + 7};
    const int lagset[] = {1, 2, 3, 64, 65, 257, 4096};
    const int ncols = 3, stride = 5;
    long long compared = 0;
    for (int weighted = 0; weighted < 2; weighted++) {
        std::vector<double> D;
        std::vector<int> w;
        std::vector<long long> start(1, 0);
        for (long long n : lens) {
            long long have = 0;
            while (have < n) {
                int wt = weighted ? (int)(rnd() * 6) : 1;
                if (have + wt > n) wt = (int)(n - have);
                for (int c = 0; c < stride; c++) D.push_back(c < ncols ? rnd() * (c + 1) : 7.0);
                w.push_back(wt);
                have += wt;
            }
            start.push_back((long long)w.size());
        }
        for (int c = 0; c < stride; c++) D.push_back(c < ncols ? rnd() : 7.0);   // one row of weight 3 T + 5
        w.push_back(3 * T + 5);
        start.push_back((long long)w.size());
        if (!weighted) {                                                          // (without weights: one more plain row)
            w.back() = 1;
        }
        const int S = (int)start.size() - 1;
        const long long R = (long long)w.size();
        std::vector<double> mean((size_t)S * ncols, 0.25);
        std::vector<long long> length(S);
        for (int nlags : lagset) {
            std::vector<double> got((size_t)S * ncols * nlags, -1.0);
            const int shapes[3][3] = {{0, 0, 0}, {50, 4, 64}, {T + 3, 1, 128}};
            for (const int *sh : shapes) {
                if (nlags > 1000 && sh[1] == 1) continue;                          // (one lag a thread: slow and no new path)
                if (as_autocov_sets(D.data(), R, stride, ncols, weighted ? w.data() : nullptr, start.data(), S,
                                    mean.data(), nlags, got.data(), length.data(), sh[0], sh[1], sh[2]))
                    return 2;
                for (int s = 0; s < S; s++)
                    for (int c = 0; c < ncols; c++) {
                        std::vector<double> y;
                        for (long long r = start[s]; r < start[s + 1]; r++)
                            for (int i = 0; i < (weighted ? w[r] : 1); i++) y.push_back(D[r * stride + c] - 0.25);
                        const long long n = (long long)y.size();
                        if (n != length[s]) return 3;
                        for (int k = 0; k < nlags; k += (nlags > 300 && k > 70 ? 97 : 1)) {
                            double acc = 0.0;
                            for (long long t = 0; t + k < n; t++) acc = __builtin_fma(y[t], y[t + k], acc);
                            const double want = n > 0 ? acc / (double)n : 0.0;
                            const double have = got[((size_t)s * ncols + c) * nlags + k];
                            if (std::memcmp(&want, &have, sizeof(double))) {
                                std::printf("series %d column %d lag %d: %.17g, want %.17g\n", s, c, k, have, want);
                                return 1;
                            }
                            compared++;
                        }
                    }
            }
        }
    }
    std::printf("%lld results equal\n", compared);
    return 0;
}
#endif
