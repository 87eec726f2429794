// datacov.hip -- the cross moment of Vs(z) and the modelled data of many sets of rows on the FP64 matrix cores
// (bh_datacov_sets).
//
// What the posterior cross-covariance of the Vs(z) profile and the modelled data (bayhunter_amd/datacov.py) needs
// beyond the two segmented scans' means: per set C = sum_r w_r dx_r dy_r^T over the centred rows, the first moments
// and the diagonal second moments of both sides.  The result and the order of its sums are defined in datacov_core.h.
//
//   datacov_weight_kernel   the pre-pass, a wave per row: the row's effective weight from its weight, its model, its err
//                     flags and ALL its S data values (datacov_effective), so that every group of data columns takes
//                     the same rows
//   datacov_kernel    a workgroup of eight waves per (block of kDepthcovBlockRows rows of one set, group of G
//                     data-column tiles): 32 threads per row walk 16 rows at a time into an LDS stage of ex = w dx (all
//                     Kp model columns) and dy (the group's 16 G data columns), the next stage while the MFMAs of this
//                     one issue; per four rows every wave issues one v_mfma_f64_16x16x4_f64 for each of its 12 tile
//                     pairs (A: ex, B: dy).  One thread per column runs the chains of r1 and q over the stage's rows:
//                     every group for its own data columns (ey = w dy is one product away), the first group for the
//                     model columns too, from a third, single stage of dx.  The block's partials go to a slab.
//   datacov_fold_kernel     one thread per (set, cell): the set's block partials added in ascending block order
//   datacov_unpack_kernel   the tiles into C [K][S]
//
// The slab holds a bounded number of blocks; a call with more takes them in runs, folding after each: the order of the
// additions is the same whatever the bound.
#include <cstring>
#include <vector>
#include "datacov_core.h"
#include "host_common.h"
#include "stats_host.h"

namespace {

using bh::u64;
typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int SR = bh::kDepthcovStageRows, WP = bh::kDepthcovWavePairs, TILE = bh::kDepthcovTile;
constexpr int kRowThreads = bh::kDepthcovThreads / SR;         // threads that share a row's columns
constexpr int kYThread0 = bh::kDepthcovThreads / 2;            // the first of the threads that own a data column
constexpr int kWeightRows = 4;                                 // rows (waves) of a pre-pass workgroup
constexpr size_t kSlabBytes = 256u << 20;                     // the most the slab of block partials takes,
constexpr long long kRunBlocks = 1024;                        // and the most blocks of one launch
constexpr size_t kMaxLds = sizeof(double) * (size_t)bh::datacov_max_lds_doubles();
static_assert(kMaxLds + 64 * sizeof(int) <= bh::kLdsLimit, "the stages of the widest K and its group fit the LDS");
static_assert(BH_DEPTHCOV_MAX_K <= kYThread0, "one thread per model column adds r1x and qx");
static_assert(16 * bh::kDatacovMaxGroupTiles <= bh::kDepthcovThreads - kYThread0, "one thread per data column of a group");
static_assert(BH_DATACOV_MAX_S % 16 == 0, "whole tiles");

struct DatacovArgs {
    const void *rows; long long stride; int width;
    const int *weff;                   // [nrows] the pre-pass' effective weights
    const double *extra; long long extra_stride;
    const double *Y; long long y_stride;        // from column col0 on
    int ndep, nextra, Kp, pitchx, Tx, S, Sp, Ty, G, Yc, pitchy, nsets;
    const long long *start, *gblk;     // [nsets + 1]: rows, blocks before set z
    long long blk0;                    // the first block of this launch
    const double *dep, *cx, *cy;       // [ndep], [nsets][K], [nsets][S]
    double *slab, *vslab;              // [blocks of the launch][Tx Ty][TILE], [..][r1x Kp | qx Kp | r1y Sp | qy Sp]
    long long *cslab;                  // [blocks of the launch][total, excluded]
};

// weff[r] = datacov_effective of row r, its S data values and nflags flags dealt to the lanes of a wave
template <typename T>
__global__ __launch_bounds__(64 * kWeightRows) void datacov_weight_kernel(const T *rows, long long stride, int width,
                                                                          const int *w, const double *Y, long long y_stride,
                                                                          int S, const int *err, long long err_stride,
                                                                          int nflags, long long nrows, int *weff, u64 *neg)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * kWeightRows + (threadIdx.x >> 6);
    if (r >= nrows) return;
    const int wr = w ? w[r] : 1;
    if (wr <= 0) {
        if (lane == 0) {
            if (wr < 0) atomicAdd(neg, 1ull);
            weff[r] = 0;
        }
        return;
    }
    bool bad = lane == 0 && bh::post_row_count(rows + r * stride, width) < 2;
    for (int f = lane; f < nflags; f += 64) bad |= err[r * err_stride + f] != 0;
    for (int j = lane; j < S; j += 64) {
        const double v = Y[r * y_stride + j];
        bad |= !(v == v);
    }
    const bool any = __any((int)bad) != 0;
    if (lane == 0) weff[r] = any ? -wr : wr;
}

template <typename T>
__global__ __launch_bounds__(bh::kDepthcovThreads) void datacov_kernel(DatacovArgs a)
{
    // dep [Kp] | cx [Kp] | cy [Yc] | 2 stages of ex [SR][pitchx] | 1 stage of dx | 2 stages of dy [SR][pitchy]
    extern __shared__ double lds[];
    __shared__ u64 s_cnt[2];                       // the block's total and excluded weight
    __shared__ int s_w[2][SR];                     // the stage rows' weights (0: the row does not count)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = a.ndep + a.nextra, Kp = a.Kp, px = a.pitchx, py = a.pitchy, Yc = a.Yc;
    double *s_dep = lds, *s_cx = lds + Kp, *s_cy = lds + 2 * Kp;
    double *exs = s_cy + Yc, *dxs = exs + 2 * SR * px, *dys = dxs + SR * px;
    const long long blk = a.blk0 + blockIdx.x;
    int z = 0, hi = a.nsets;                       // gblk[z] <= blk < gblk[z + 1]
    while (hi - z > 1) {
        const int mid = z + (hi - z) / 2;
        if (a.gblk[mid] <= blk) z = mid; else hi = mid;
    }
    const long long r0 = a.start[z] + (blk - a.gblk[z]) * bh::kDepthcovBlockRows;
    const long long left = a.start[z + 1] - r0;
    const int nrows = left < bh::kDepthcovBlockRows ? (int)left : bh::kDepthcovBlockRows;
    const int nst = (nrows + SR - 1) / SR;
    const int grp = (int)blockIdx.y, j0 = grp * Yc;               // the group's first data column
    const int gtiles = a.Ty - grp * a.G < a.G ? a.Ty - grp * a.G : a.G;
    const int npl = a.Tx * gtiles;                 // tile pairs of this group
    const bool first_group = grp == 0;             // the group that also adds the model side's sums and the weights
    for (int c = tid; c < Kp; c += bh::kDepthcovThreads) {
        s_dep[c] = c < a.ndep ? a.dep[c] : 0.0;
        s_cx[c] = c < K ? a.cx[(size_t)z * K + c] : 0.0;
    }
    for (int c = tid; c < Yc; c += bh::kDepthcovThreads) s_cy[c] = j0 + c < a.S ? a.cy[(size_t)z * a.S + j0 + c] : 0.0;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();

    int ti[WP], tj[WP];
    double4_t acc[WP];
    const int pbase = wave * WP;
#pragma unroll
    for (int q = 0; q < WP; q++) {
        ti[q] = tj[q] = 0;                         // a pair past the last: tile (0, 0) again, never written
        if (pbase + q < npl) {
            ti[q] = (pbase + q) % a.Tx;
            tj[q] = (pbase + q) / a.Tx;
        }
        acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
    }
    const int srow = tid / kRowThreads, seg = tid % kRowThreads;
    const T *rows = (const T *)a.rows;
    auto stage = [&](int s) {
        const int i = s * SR + srow;
        const long long r = r0 + i;
        const int weff = i < nrows ? a.weff[r] : 0;
        const bool in = weff > 0;
        if (seg == 0) {
            s_w[s & 1][srow] = in ? weff : 0;
            if (first_group && weff != 0) atomicAdd(&s_cnt[in ? 0 : 1], (u64)(in ? weff : -(long long)weff));
        }
        bh::datacov_row_x<T>(in ? rows + r * a.stride : nullptr, a.width, weff,
                             in && a.nextra ? a.extra + r * a.extra_stride : nullptr, a.ndep, a.nextra, s_dep, s_cx, seg,
                             Kp, kRowThreads, exs + (size_t)(s & 1) * (SR * px) + srow * px,
                             first_group ? dxs + srow * px : nullptr);
        bh::datacov_row_y(in ? a.Y + r * a.y_stride : nullptr, weff, a.S, s_cy, j0, seg, Yc, kRowThreads,
                          dys + (size_t)(s & 1) * (SR * py) + srow * py);
    };
    const int mrow = lane & 15, kq = lane >> 4;
    const int ycol = tid - kYThread0;              // the data column of the group this thread sums, if any
    double r1 = 0.0, qq = 0.0;
    if (nst > 0) stage(0);
    __syncthreads();
    for (int s = 0; s < nst; s++) {
        const double *eP = exs + (size_t)(s & 1) * (SR * px), *yP = dys + (size_t)(s & 1) * (SR * py);
        if (first_group && tid < Kp) {
            for (int i = 0; i < SR; i++) {
                const double e = eP[i * px + tid];
                r1 = r1 + e;
                qq = __builtin_fma(e, dxs[i * px + tid], qq);
            }
        } else if (ycol >= 0 && ycol < Yc) {
            for (int i = 0; i < SR; i++) {
                const double d = yP[i * py + ycol], e = (double)s_w[s & 1][i] * d;
                r1 = r1 + e;
                qq = __builtin_fma(e, d, qq);
            }
        }
        if (first_group) __syncthreads();          // dx was read: the next stage may overwrite it
        if (s + 1 < nst) stage(s + 1);             // the other stage: free since the last barrier
#pragma unroll
        for (int ks = 0; ks < SR / 4; ks++) {
            const int ox = (ks * 4 + kq) * px + mrow, oy = (ks * 4 + kq) * py + mrow;
#pragma unroll
            for (int q = 0; q < WP; q++)
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(eP[ox + 16 * ti[q]], yP[oy + 16 * tj[q]], acc[q], 0, 0, 0);
        }
        __syncthreads();
    }
    const int npairs = a.Tx * a.Ty;
    double *out = a.slab + ((size_t)blockIdx.x * npairs + (size_t)grp * a.G * a.Tx) * TILE;
#pragma unroll
    for (int q = 0; q < WP; q++)
        if (pbase + q < npl) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) out[(size_t)(pbase + q) * TILE + reg * 64 + lane] = acc[q][reg];
        }
    double *v = a.vslab + (size_t)blockIdx.x * (2 * Kp + 2 * a.Sp);
    if (first_group && tid < Kp) {
        v[tid] = r1;
        v[Kp + tid] = qq;
    } else if (ycol >= 0 && ycol < Yc && j0 + ycol < a.Sp) {
        v[2 * Kp + j0 + ycol] = r1;
        v[2 * Kp + a.Sp + j0 + ycol] = qq;
    }
    if (first_group && tid < 2) a.cslab[(size_t)blockIdx.x * 2 + tid] = (long long)s_cnt[tid];
}

// cells of a set: Tx Ty TILE of C, 2 Kp + 2 Sp of the sums, two weights.  Blocks [blk0, blk1) are in the slab.
__global__ void datacov_fold_kernel(DatacovArgs a, int z0, int nz, long long blk1, double *Cacc, double *vacc,
                                    long long *cacc)
{
    const long long ncell = (long long)a.Tx * a.Ty * TILE, nv = 2 * a.Kp + 2 * a.Sp, per = ncell + nv + 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * nz) return;
    const int z = z0 + (int)(i / per);
    const long long c = i % per;
    const long long b0 = a.gblk[z] > a.blk0 ? a.gblk[z] : a.blk0, b1 = a.gblk[z + 1] < blk1 ? a.gblk[z + 1] : blk1;
    if (c < ncell) {
        double s = Cacc[(size_t)z * ncell + c];
        for (long long b = b0; b < b1; b++) s = s + a.slab[(size_t)(b - a.blk0) * ncell + c];
        Cacc[(size_t)z * ncell + c] = s;
    } else if (c < ncell + nv) {
        const long long k = c - ncell;
        double s = vacc[(size_t)z * nv + k];
        for (long long b = b0; b < b1; b++) s = s + a.vslab[(size_t)(b - a.blk0) * nv + k];
        vacc[(size_t)z * nv + k] = s;
    } else {
        const int k = (int)(c - ncell - nv);
        long long s = cacc[(size_t)z * 2 + k];
        for (long long b = b0; b < b1; b++) s += a.cslab[(size_t)(b - a.blk0) * 2 + k];
        cacc[(size_t)z * 2 + k] = s;
    }
}

// the tiles into C [nsets][K][S]
__global__ void datacov_unpack_kernel(const double *Cacc, int nsets, int K, int S, int Tx, int npairs, double *C)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nsets * npairs * TILE) return;
    const int cell = (int)(i % TILE), p = (int)(i / TILE % npairs);
    const size_t z = (size_t)(i / ((long long)npairs * TILE));
    const int m = cell >> 4, n = cell & 15;
    const int row = 16 * (p % Tx) + m, col = 16 * (p / Tx) + n;
    if (row >= K || col >= S) return;
    C[(z * K + row) * S + col] = Cacc[(z * npairs + p) * TILE + bh::depthcov_acc_slot(m, n)];
}

}  // namespace

extern "C" int bh_datacov_sets(const void *rows, int fp64, long long nrows, long long stride, int width,
                               const int *weights, const double *extra, long long extra_stride, int nextra,
                               const double *Y, long long y_stride, int col0, int S, const int *err, long long err_stride,
                               int nflags, const long long *set_start, int nsets, const double *dep, int ndep,
                               const double *cx, const double *cy, double *C, double *r1x, double *r1y, double *qx,
                               double *qy, long long *total, long long *excluded, void *stream)
{
    if (!rows || nrows < 1) return bh::fail_arg_("bh_datacov_sets: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_datacov_sets: more than 2^32 rows");
    if (width < 2 || stride < width) return bh::fail_arg_("bh_datacov_sets: width >= 2 and stride >= width");
    if (ndep < 1 || !dep) return bh::fail_arg_("bh_datacov_sets: ndep >= 1 depths");
    if (!bh::ascending(dep, ndep)) return bh::fail_arg_("bh_datacov_sets: dep must be ascending");
    if (nextra < 0 || (nextra > 0 && (!extra || extra_stride < nextra)))
        return bh::fail_arg_("bh_datacov_sets: extra [nrows][nextra] with extra_stride >= nextra");
    if ((long long)ndep + nextra > BH_DEPTHCOV_MAX_K) return bh::fail_arg_("bh_datacov_sets: K = ndep + nextra above 256");
    if (S < 1 || S > BH_DATACOV_MAX_S) return bh::fail_arg_("bh_datacov_sets: 1 <= S <= 1024 data columns");
    if (!Y || col0 < 0 || y_stride < (long long)col0 + S)
        return bh::fail_arg_("bh_datacov_sets: Y [nrows][y_stride] with col0 >= 0 and y_stride >= col0 + S");
    if (nflags < 0 || (nflags > 0 && (!err || err_stride < nflags)))
        return bh::fail_arg_("bh_datacov_sets: err [nrows][nflags] with err_stride >= nflags");
    if (nsets < 1) return bh::fail_arg_("bh_datacov_sets: one set at least");
    if (int rc = bh::check_set_start("bh_datacov_sets", set_start, nsets, nrows)) return rc;
    if (!cx || !cy || !C || !r1x || !r1y || !qx || !qy || !total || !excluded)
        return bh::fail_arg_("bh_datacov_sets: cx, cy, C, r1x, r1y, qx, qy, total and excluded");
    const int K = ndep + nextra, Kp = bh::depthcov_kp(K), Tx = Kp / 16, Sp = bh::depthcov_kp(S), Ty = Sp / 16;
    const int npairs = Tx * Ty, G = bh::datacov_group_tiles(Tx), Yc = 16 * G, nv = 2 * Kp + 2 * Sp;
    const size_t Z = (size_t)nsets, ncell = (size_t)npairs * TILE;
    std::vector<long long> gblk(Z + 1, 0);
    for (int z = 0; z < nsets; z++) gblk[z + 1] = gblk[z] + bh::depthcov_blocks(set_start[z + 1] - set_start[z]);
    const long long nblk = gblk[Z];
    if ((Z * (ncell + nv + 2) + 255) / 256 > 0x7fffffffull)
        return bh::fail_arg_("bh_datacov_sets: more than 2^31 - 1 workgroups in one launch");
    if (int rc = bh::require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    u64 neg = 0;                                   // before tmp: tmp drains the stream on every return, this one outlives it
    bh::CallBufs tmp(st);
    DatacovArgs a;
    std::memset(&a, 0, sizeof(a));
    long long per_run = (long long)(kSlabBytes / (sizeof(double) * ncell));    // blocks the slab holds at a time
    per_run = per_run < 1 ? 1 : per_run > kRunBlocks ? kRunBlocks : per_run;
    const long long run = nblk < per_run ? nblk : per_run;
    long long *dstart = nullptr, *dgblk = nullptr, *cacc = nullptr;
    double *ddep = nullptr, *dcx = nullptr, *dcy = nullptr, *Cacc = nullptr, *vacc = nullptr, *dC = nullptr;
    int *dweff = nullptr;
    u64 *dneg = nullptr;
    BH_HIP(tmp.alloc(dstart, Z + 1));
    BH_HIP(tmp.alloc(dgblk, Z + 1));
    BH_HIP(tmp.alloc(ddep, (size_t)ndep));
    BH_HIP(tmp.alloc(dcx, Z * K));
    BH_HIP(tmp.alloc(dcy, Z * S));
    BH_HIP(tmp.alloc(dweff, (size_t)nrows));
    BH_HIP(tmp.alloc(a.slab, (size_t)run * ncell));
    BH_HIP(tmp.alloc(a.vslab, (size_t)run * nv));
    BH_HIP(tmp.alloc(a.cslab, (size_t)run * 2));
    BH_HIP(tmp.alloc(dneg, 1));
    BH_HIP(tmp.alloc(Cacc, Z * ncell));
    BH_HIP(tmp.alloc(vacc, Z * nv));
    BH_HIP(tmp.alloc(cacc, Z * 2));
    BH_HIP(tmp.alloc(dC, Z * K * S));
    BH_HIP(hipMemcpyAsync(dstart, set_start, sizeof(long long) * (Z + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dgblk, gblk.data(), sizeof(long long) * (Z + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(ddep, dep, sizeof(double) * ndep, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dcx, cx, sizeof(double) * Z * K, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dcy, cy, sizeof(double) * Z * S, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemsetAsync(dneg, 0, sizeof(u64), st));
    BH_HIP(hipMemsetAsync(Cacc, 0, sizeof(double) * Z * ncell, st));
    BH_HIP(hipMemsetAsync(vacc, 0, sizeof(double) * Z * nv, st));
    BH_HIP(hipMemsetAsync(cacc, 0, sizeof(long long) * Z * 2, st));
    const dim3 wgrid((unsigned)((nrows + kWeightRows - 1) / kWeightRows));
    if (fp64)
        hipLaunchKernelGGL(datacov_weight_kernel<double>, wgrid, dim3(64 * kWeightRows), 0, st, (const double *)rows, stride,
                           width, weights, Y + col0, y_stride, S, err, err_stride, nflags, nrows, dweff, dneg);
    else
        hipLaunchKernelGGL(datacov_weight_kernel<float>, wgrid, dim3(64 * kWeightRows), 0, st, (const float *)rows, stride,
                           width, weights, Y + col0, y_stride, S, err, err_stride, nflags, nrows, dweff, dneg);
    BH_HIP(hipGetLastError());
    a.rows = rows; a.stride = stride; a.width = width;
    a.weff = dweff;
    a.extra = extra; a.extra_stride = extra_stride;
    a.Y = Y + col0; a.y_stride = y_stride;
    a.ndep = ndep; a.nextra = nextra; a.Kp = Kp; a.pitchx = bh::datacov_pitch(Kp); a.Tx = Tx;
    a.S = S; a.Sp = Sp; a.Ty = Ty; a.G = G; a.Yc = Yc; a.pitchy = bh::datacov_pitch(Yc);
    a.nsets = nsets;
    a.start = dstart; a.gblk = dgblk;
    a.dep = ddep; a.cx = dcx; a.cy = dcy;
    const size_t dyn = sizeof(double) * (size_t)bh::datacov_lds_doubles(Kp, Yc);
    const void *fn = fp64 ? (const void *)datacov_kernel<double> : (const void *)datacov_kernel<float>;
    BH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
    const unsigned groups = (unsigned)((Ty + G - 1) / G);
    int z0 = 0;                                    // the first set with a block at or after blk0
    for (long long b0 = 0; b0 < nblk; b0 += run) {
        const long long b1 = b0 + run < nblk ? b0 + run : nblk;
        a.blk0 = b0;
        const dim3 grid((unsigned)(b1 - b0), groups);
        if (fp64) hipLaunchKernelGGL(datacov_kernel<double>, grid, dim3(bh::kDepthcovThreads), dyn, st, a);
        else hipLaunchKernelGGL(datacov_kernel<float>, grid, dim3(bh::kDepthcovThreads), dyn, st, a);
        BH_HIP(hipGetLastError());
        while (gblk[z0 + 1] <= b0) z0++;
        int z1 = z0;                               // the last set with a block before b1
        while (z1 + 1 < nsets && gblk[z1 + 1] < b1) z1++;
        const long long cells = (long long)(z1 - z0 + 1) * (long long)(ncell + nv + 2);
        hipLaunchKernelGGL(datacov_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a, z0,
                           z1 - z0 + 1, b1, Cacc, vacc, cacc);
        BH_HIP(hipGetLastError());
    }
    BH_HIP(hipMemsetAsync(dC, 0, sizeof(double) * Z * K * S, st));
    hipLaunchKernelGGL(datacov_unpack_kernel, dim3((unsigned)((Z * ncell + 255) / 256)), dim3(256), 0, st,
                       (const double *)Cacc, nsets, K, S, Tx, npairs, dC);
    BH_HIP(hipGetLastError());
    std::vector<double> hv(Z * nv);
    std::vector<long long> hc(Z * 2);
    BH_HIP(hipMemcpyAsync(&neg, dneg, sizeof(u64), hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(C, dC, sizeof(double) * Z * K * S, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(hv.data(), vacc, sizeof(double) * Z * nv, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(hc.data(), cacc, sizeof(long long) * Z * 2, hipMemcpyDeviceToHost, st));
    BH_HIP(hipStreamSynchronize(st));
    if (neg) return bh::fail_arg_("bh_datacov_sets: negative weight");
    for (size_t z = 0; z < Z; z++) {
        const double *v = hv.data() + z * nv;
        for (int k = 0; k < K; k++) {
            r1x[z * K + k] = v[k];
            qx[z * K + k] = v[Kp + k];
        }
        for (int j = 0; j < S; j++) {
            r1y[z * S + j] = v[2 * Kp + j];
            qy[z * S + j] = v[2 * Kp + Sp + j];
        }
        total[z] = hc[z * 2];
        excluded[z] = hc[z * 2 + 1];
    }
    return BH_OK;
}
