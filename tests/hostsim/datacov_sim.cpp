// datacov_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the core of the cross moment of Vs(z) and the modelled data (bayhunter_amd/csrc/datacov_core.h) with g++ so
// that the CPU tier computes what bh_datacov_sets returns with the kernel's blocking -- the effective weight of every row
// decided first from all S data columns (datacov_effective), blocks counted from the set's first row, stage rows made by
// datacov_row_x / datacov_row_y, every tile pair, block partials added in ascending order from 0.0 -- against the numpy
// restatement (tests/datacov_ref.py).  Where the device issues one MFMA per four rows, the twin runs one fma chain per
// cell over the rows in ascending order; whether the two round alike is measured by the GPU tier, not assumed.
#define BH_HOSTSIM 1
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/datacov_core.h"

namespace {

inline bool ascending(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!(v[i] == v[i]) || (i && !(v[i - 1] < v[i]))) return false;
    return true;
}

struct Out {
    double *C, *r1x, *r1y, *qx, *qy;
    long long *total, *excluded;
};

template <typename T>
int walk(const T *rows, long long stride, int width, const int *weights, const double *extra, long long extra_stride,
         int nextra, const double *Y, long long y_stride, int S, const int *err, long long err_stride, int nflags,
         const long long *start, int nsets, const double *dep, int ndep, const double *cx, const double *cy, Out o,
         int block_rows)
{
    const int K = ndep + nextra, Kp = bh::depthcov_kp(K), Sp = bh::depthcov_kp(S);
    const long long nrows = start[nsets];
    std::vector<int> weff((size_t)nrows);
    for (long long r = 0; r < nrows; r++) {        // the pre-pass
        const int w = weights ? weights[r] : 1;
        if (w < 0) return 1;
        weff[(size_t)r] = bh::datacov_effective<T>(rows + r * stride, width, w, Y + r * y_stride, S,
                                                   nflags ? err + r * err_stride : nullptr, nflags);
    }
    std::vector<double> ex((size_t)block_rows * Kp), dx((size_t)block_rows * Kp), dy((size_t)block_rows * Sp);
    std::vector<int> wb(block_rows);
    std::vector<double> sdep(Kp, 0.0), scx(Kp, 0.0), scy(Sp, 0.0);
    for (int c = 0; c < ndep; c++) sdep[c] = dep[c];
    for (int z = 0; z < nsets; z++) {
        std::vector<double> Cacc((size_t)Kp * Sp, 0.0), r1xa(Kp, 0.0), qxa(Kp, 0.0), r1ya(Sp, 0.0), qya(Sp, 0.0);
        long long tot = 0, exc = 0;
        for (int c = 0; c < K; c++) scx[c] = cx[(size_t)z * K + c];
        for (int j = 0; j < S; j++) scy[j] = cy[(size_t)z * S + j];
        for (long long r0 = start[z]; r0 < start[z + 1]; r0 += block_rows) {
            const long long left = start[z + 1] - r0;
            const int n = left < block_rows ? (int)left : block_rows;
            for (int i = 0; i < n; i++) {
                const long long r = r0 + i;
                const int we = weff[(size_t)r];
                const bool in = we > 0;
                wb[i] = in ? we : 0;
                if (in) tot += we; else exc -= we;
                // the columns of a row dealt to 32 walks, as the kernel deals them to its threads
                for (int seg = 0; seg < 32; seg++) {
                    bh::datacov_row_x<T>(in ? rows + r * stride : nullptr, width, we,
                                         in && nextra ? extra + r * extra_stride : nullptr, ndep, nextra, sdep.data(),
                                         scx.data(), seg, Kp, 32, &ex[(size_t)i * Kp], &dx[(size_t)i * Kp]);
                    bh::datacov_row_y(in ? Y + r * y_stride : nullptr, we, S, scy.data(), 0, seg, Sp, 32,
                                      &dy[(size_t)i * Sp]);
                }
            }
            for (int c = 0; c < Kp; c++) {
                double a1 = 0.0, aq = 0.0;
                for (int i = 0; i < n; i++) {
                    const double e = ex[(size_t)i * Kp + c];
                    a1 = a1 + e;
                    aq = __builtin_fma(e, dx[(size_t)i * Kp + c], aq);
                }
                r1xa[c] = r1xa[c] + a1;
                qxa[c] = qxa[c] + aq;
            }
            for (int j = 0; j < Sp; j++) {
                double a1 = 0.0, aq = 0.0;
                for (int i = 0; i < n; i++) {
                    const double d = dy[(size_t)i * Sp + j], e = (double)wb[i] * d;
                    a1 = a1 + e;
                    aq = __builtin_fma(e, d, aq);
                }
                r1ya[j] = r1ya[j] + a1;
                qya[j] = qya[j] + aq;
            }
            for (int c = 0; c < K; c++)
                for (int j = 0; j < S; j++) {
                    double acc = 0.0;
                    for (int i = 0; i < n; i++) acc = __builtin_fma(ex[(size_t)i * Kp + c], dy[(size_t)i * Sp + j], acc);
                    Cacc[(size_t)c * Sp + j] = Cacc[(size_t)c * Sp + j] + acc;
                }
        }
        for (int c = 0; c < K; c++) {
            for (int j = 0; j < S; j++) o.C[((size_t)z * K + c) * S + j] = Cacc[(size_t)c * Sp + j];
            o.r1x[(size_t)z * K + c] = r1xa[c];
            o.qx[(size_t)z * K + c] = qxa[c];
        }
        for (int j = 0; j < S; j++) {
            o.r1y[(size_t)z * S + j] = r1ya[j];
            o.qy[(size_t)z * S + j] = qya[j];
        }
        o.total[z] = tot;
        o.excluded[z] = exc;
    }
    return 0;
}

}  // namespace

extern "C" int dcs_block_rows(void) { return bh::kDepthcovBlockRows; }
extern "C" int dcs_max_k(void) { return BH_DEPTHCOV_MAX_K; }
extern "C" int dcs_max_s(void) { return BH_DATACOV_MAX_S; }
// data columns of one group on blockIdx.y for K model columns
extern "C" int dcs_group_cols(int K) { return 16 * bh::datacov_group_tiles(bh::depthcov_kp(K) / 16); }
extern "C" int dcs_lds_bytes(int K) { return 8 * bh::datacov_lds_doubles(bh::depthcov_kp(K), dcs_group_cols(K)); }
extern "C" int dcs_max_lds_bytes(void) { return 8 * bh::datacov_max_lds_doubles(); }

// bh_datacov_sets as its kernels order the sums.  block_rows: 0 for the library's.  -> 0, 1 for a negative weight, 2
// for arguments the library refuses
extern "C" int dcs_datacov_sets(const void *rows, int fp64, long long nrows, long long stride, int width,
                                const int *weights, const double *extra, long long extra_stride, int nextra,
                                const double *Y, long long y_stride, int col0, int S, const int *err, long long err_stride,
                                int nflags, const long long *set_start, int nsets, const double *dep, int ndep,
                                const double *cx, const double *cy, double *C, double *r1x, double *r1y, double *qx,
                                double *qy, long long *total, long long *excluded, int block_rows)
{
    if (!rows || nrows < 1 || width < 2 || stride < width || ndep < 1 || nextra < 0 || nsets < 1) return 2;
    if (ndep + nextra > BH_DEPTHCOV_MAX_K || !ascending(dep, ndep)) return 2;
    if (!Y || S < 1 || S > BH_DATACOV_MAX_S || col0 < 0 || y_stride < (long long)col0 + S || nflags < 0) return 2;
    if (set_start[0] != 0 || set_start[nsets] != nrows) return 2;
    for (int z = 0; z < nsets; z++)
        if (set_start[z] > set_start[z + 1]) return 2;
    if (block_rows < 1) block_rows = bh::kDepthcovBlockRows;
    Out o = {C, r1x, r1y, qx, qy, total, excluded};
    if (fp64)
        return walk<double>((const double *)rows, stride, width, weights, extra, extra_stride, nextra, Y + col0, y_stride, S,
                            err, err_stride, nflags, set_start, nsets, dep, ndep, cx, cy, o, block_rows);
    return walk<float>((const float *)rows, stride, width, weights, extra, extra_stride, nextra, Y + col0, y_stride, S, err,
                       err_stride, nflags, set_start, nsets, dep, ndep, cx, cy, o, block_rows);
}
