// depthcov_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the core of the depth-to-depth second moment (bayhunter_amd/csrc/depthcov_core.h) with g++ so that the CPU
// tier computes S, r1 and total of bh_depthcov_sets with the kernel's blocking -- blocks counted from the set's first
// row, stage rows made by depthcov_row, the tile pairs of the upper triangle with the diagonal tiles' convention, block
// partials added in ascending order from 0.0 -- against the numpy restatement (tests/depthcov_ref.py).  Where the device
// issues one MFMA per four rows, the twin runs one fma chain per cell over the rows in ascending order; whether the two
// round alike is measured by the GPU tier, not assumed.
#define BH_HOSTSIM 1
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/depthcov_core.h"

namespace {

inline bool ascending(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!(v[i] == v[i]) || (i && !(v[i - 1] < v[i]))) return false;
    return true;
}

template <typename T>
int walk(const T *rows, long long stride, int width, const int *weights, const double *extra, long long extra_stride,
         int nextra, const long long *start, int nsets, const double *dep, int ndep, const double *center, double *S,
         double *r1, long long *total, int block_rows)
{
    const int K = ndep + nextra, Kp = bh::depthcov_kp(K), Tn = Kp / 16, npairs = bh::depthcov_npairs(Tn);
    std::vector<double> d((size_t)block_rows * Kp), e((size_t)block_rows * Kp), tile(bh::kDepthcovTile);
    std::vector<double> sdep(Kp, 0.0), scen(Kp, 0.0);
    for (int c = 0; c < ndep; c++) sdep[c] = dep[c];
    for (int z = 0; z < nsets; z++) {
        double *Sz = S + (size_t)z * K * K, *rz = r1 + (size_t)z * K;
        std::vector<double> Sacc((size_t)npairs * bh::kDepthcovTile, 0.0), racc(Kp, 0.0);
        long long tot = 0;
        for (int c = 0; c < K; c++) scen[c] = center[(size_t)z * K + c];
        for (long long r0 = start[z]; r0 < start[z + 1]; r0 += block_rows) {
            const long long left = start[z + 1] - r0;
            const int n = left < block_rows ? (int)left : block_rows;
            for (int i = 0; i < n; i++) {
                const long long r = r0 + i;
                const int w = weights ? weights[r] : 1;
                if (w < 0) return 1;
                // the columns of a row dealt to 32 walks, as the kernel deals them to its threads
                bool in = false;
                for (int seg = 0; seg < 32; seg++)
                    in = bh::depthcov_row<T>(rows + r * stride, width, w, nextra ? extra + r * extra_stride : nullptr, ndep,
                                             nextra, sdep.data(), scen.data(), seg, Kp, 32, &d[(size_t)i * Kp],
                                             &e[(size_t)i * Kp]);
                if (in) tot += w;
            }
            for (int c = 0; c < Kp; c++) {
                double acc = 0.0;
                for (int i = 0; i < n; i++) acc = acc + e[(size_t)i * Kp + c];
                racc[c] = racc[c] + acc;
            }
            for (int p = 0; p < npairs; p++) {
                int ti, tj;
                bh::depthcov_pair(Tn, p, &ti, &tj);
                for (int m = 0; m < 16; m++)
                    for (int nn = 0; nn < 16; nn++) {
                        double acc = 0.0;
                        for (int i = 0; i < n; i++)
                            acc = __builtin_fma(e[(size_t)i * Kp + 16 * ti + m], d[(size_t)i * Kp + 16 * tj + nn], acc);
                        double &s = Sacc[(size_t)p * bh::kDepthcovTile + bh::depthcov_acc_slot(m, nn)];
                        s = s + acc;
                    }
            }
        }
        for (int p = 0; p < npairs; p++) {
            int ti, tj;
            bh::depthcov_pair(Tn, p, &ti, &tj);
            for (int m = 0; m < 16; m++)
                for (int nn = 0; nn < 16; nn++) {
                    const int row = 16 * ti + m, col = 16 * tj + nn;
                    if (row >= K || col >= K || (ti == tj && nn < m)) continue;
                    const double v = Sacc[(size_t)p * bh::kDepthcovTile + bh::depthcov_acc_slot(m, nn)];
                    Sz[(size_t)row * K + col] = v;
                    Sz[(size_t)col * K + row] = v;
                }
        }
        for (int c = 0; c < K; c++) rz[c] = racc[c];
        total[z] = tot;
    }
    return 0;
}

}  // namespace

extern "C" int ds_block_rows(void) { return bh::kDepthcovBlockRows; }
extern "C" int ds_max_k(void) { return BH_DEPTHCOV_MAX_K; }
extern "C" int ds_lds_bytes(int K) { return 8 * bh::depthcov_lds_doubles(bh::depthcov_kp(K)); }
extern "C" int ds_group_pairs(void) { return bh::kDepthcovGroupPairs; }
extern "C" int ds_npairs(int K) { return bh::depthcov_npairs(bh::depthcov_kp(K) / 16); }
extern "C" void ds_pair(int T, int p, int *i, int *j) { bh::depthcov_pair(T, p, i, j); }
extern "C" int ds_acc_slot(int m, int n) { return bh::depthcov_acc_slot(m, n); }

// bh_depthcov_sets as its kernels order the sums.  block_rows: 0 for the library's.  -> 0, 1 for a negative weight, 2
// for arguments the library refuses
extern "C" int ds_depthcov_sets(const void *rows, int fp64, long long nrows, long long stride, int width,
                                const int *weights, const double *extra, long long extra_stride, int nextra,
                                const long long *set_start, int nsets, const double *dep, int ndep, const double *center,
                                double *S, double *r1, long long *total, int block_rows)
{
    if (!rows || nrows < 1 || width < 2 || stride < width || ndep < 1 || nextra < 0 || nsets < 1) return 2;
    if (ndep + nextra > BH_DEPTHCOV_MAX_K || !ascending(dep, ndep)) return 2;
    if (set_start[0] != 0 || set_start[nsets] != nrows) return 2;
    for (int z = 0; z < nsets; z++)
        if (set_start[z] > set_start[z + 1]) return 2;
    if (block_rows < 1) block_rows = bh::kDepthcovBlockRows;
    const int K = ndep + nextra;
    std::memset(S, 0, sizeof(double) * (size_t)nsets * K * K);
    if (fp64)
        return walk<double>((const double *)rows, stride, width, weights, extra, extra_stride, nextra, set_start, nsets,
                            dep, ndep, center, S, r1, total, block_rows);
    return walk<float>((const float *)rows, stride, width, weights, extra, extra_stride, nextra, set_start, nsets, dep, ndep,
                       center, S, r1, total, block_rows);
}
