// interfaces_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the per-row core of the discontinuity statistics (bayhunter_amd/csrc/interfaces_core.h) with g++ and
// replays what interfaces.hip does with it on the host: the integer cells through the same walk, taken in groups of
// `group` depth bins as the kernel takes them when its LDS is short (0: all at once), and the two floating-point sums
// in the order interfaces_core.h states (blocks of a set, waves, trips, interface index, lanes).  The CPU tier holds
// it against the numpy restatement (tests/interfaces_ref.py), the GPU tier holds the kernels against it.
#define BH_HOSTSIM 1
#include <cmath>
#include <vector>
#include "../../bayhunter_amd/csrc/interfaces_core.h"

namespace {

struct PlainAdd {
    void operator()(uint64_t *cell, uint64_t w) const { *cell += w; }
};

// Σ of one pass over the rows [r0, r1) of a set -> out[nbd]
template <typename T>
void moment_pass(const T *rows, long stride, int width, const int *w, long r0, long r1, const double *dedges, int nde,
                 const double *mean, double *out)
{
    const int nbd = nde - 1;
    for (int d = 0; d < nbd; d++) out[d] = 0.0;
    std::vector<double> acc((size_t)bh::kIfWaves * nbd);
    for (long b0 = r0; b0 < r1; b0 += bh::kIfRowsPerBlock) {
        for (double &v : acc) v = 0.0;
        for (int wave = 0; wave < bh::kIfWaves; wave++) {
            double *mine = acc.data() + (size_t)wave * nbd;
            for (int t = 0; t < bh::kIfTrips; t++) {
                bh::PostWalk<T> wk[bh::kIfWave];
                double wt[bh::kIfWave];
                bool any = false;
                for (int lane = 0; lane < bh::kIfWave; lane++) {
                    const long r = b0 + (long)t * bh::kIfThreads + wave * bh::kIfWave + lane;
                    const int wr = r < r1 ? (w ? w[r] : 1) : 0;
                    const T *row = rows + (r < r1 ? r : r0) * stride;
                    wk[lane].init(row, wr > 0 ? bh::post_row_count(row, width) : 0);
                    wt[lane] = (double)wr;
                    any = any || wk[lane].has_interface();
                }
                while (any) {
                    any = false;
                    for (int lane = 0; lane < bh::kIfWave; lane++) {
                        if (!wk[lane].has_interface()) continue;
                        const int d = bh::post_bin(dedges, nde, wk[lane].D);
                        if (d >= 0) mine[d] = mine[d] + bh::interfaces_term(wt[lane], bh::interfaces_jump(wk[lane]), mean, d);
                        wk[lane].cross();
                        any = any || wk[lane].has_interface();
                    }
                }
            }
        }
        for (int d = 0; d < nbd; d++)
            out[d] = out[d] + (((acc[d] + acc[nbd + d]) + acc[2 * (size_t)nbd + d]) + acc[3 * (size_t)nbd + d]);
    }
}

template <typename T>
int sets(const T *rows, long R, long stride, int width, const int *w, const long long *start, int nsets,
         const double *dedges, int nde, const double *jedges, int nje, int group, long long *total, long long *fields,
         long long *hist, double *jsum, double *jsq)
{
    const int nbd = nde - 1, nbj = nje > 1 ? nje - 1 : 0, per = bh::IF_FIELDS + nbj;
    if (group < 1 || group > nbd) group = nbd;
    for (long r = 0; r < R; r++)
        if (w && w[r] < 0) return 1;
    std::vector<uint64_t> tab((size_t)nbd * per);
    std::vector<double> sum(nbd), mu(nbd), sq(nbd);
    for (int z = 0; z < nsets; z++) {
        const long r0 = (long)start[z], r1 = (long)start[z + 1];
        for (uint64_t &c : tab) c = 0;
        long long tot = 0;
        for (int d0 = 0; d0 < nbd; d0 += group) {
            const int d1 = d0 + group < nbd ? d0 + group : nbd;
            for (long r = r0; r < r1; r++) {
                const int wr = w ? w[r] : 1;
                if (d0 == 0) tot += wr;
                if (wr <= 0) continue;
                bh::interfaces_row(rows + r * stride, width, (uint64_t)wr, dedges, nde, jedges, nje, d0, d1,
                                   tab.data() + (size_t)d0 * per, PlainAdd());
            }
        }
        total[z] = tot;
        for (int d = 0; d < nbd; d++) {
            for (int f = 0; f < bh::IF_FIELDS; f++)      // fields[field][set][depth bin]
                fields[((size_t)f * nsets + z) * nbd + d] = (long long)tab[(size_t)d * per + f];
            for (int j = 0; j < nbj; j++) hist[((size_t)z * nbd + d) * nbj + j] = (long long)tab[(size_t)d * per + bh::IF_FIELDS + j];
        }
        moment_pass(rows, stride, width, w, r0, r1, dedges, nde, (const double *)nullptr, sum.data());
        for (int d = 0; d < nbd; d++) {
            const uint64_t c = tab[(size_t)d * per + bh::IF_COUNT];
            mu[d] = c ? sum[d] / (double)c : std::nan("");
        }
        moment_pass(rows, stride, width, w, r0, r1, dedges, nde, mu.data(), sq.data());
        for (int d = 0; d < nbd; d++) {
            jsum[(size_t)z * nbd + d] = tot ? sum[d] : std::nan("");
            jsq[(size_t)z * nbd + d] = tot ? sq[d] : std::nan("");
        }
    }
    return 0;
}

}  // namespace

extern "C" int ifs_sets32(const float *rows, long R, long stride, int width, const int *w, const long long *start,
                          int nsets, const double *dedges, int nde, const double *jedges, int nje, int group,
                          long long *total, long long *fields, long long *hist, double *jsum, double *jsq)
{
    return sets(rows, R, stride, width, w, start, nsets, dedges, nde, jedges, nje, group, total, fields, hist, jsum, jsq);
}
extern "C" int ifs_sets64(const double *rows, long R, long stride, int width, const int *w, const long long *start,
                          int nsets, const double *dedges, int nde, const double *jedges, int nje, int group,
                          long long *total, long long *fields, long long *hist, double *jsum, double *jsq)
{
    return sets(rows, R, stride, width, w, start, nsets, dedges, nde, jedges, nje, group, total, fields, hist, jsum, jsq);
}
extern "C" int ifs_blocks_of(long long nrows) { return bh::interfaces_blocks_of(nrows); }
extern "C" int ifs_group(int nbd, int nbj) { return bh::interfaces_group(nbd, nbj); }
extern "C" int ifs_rows_per_block(void) { return bh::kIfRowsPerBlock; }
