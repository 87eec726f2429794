// depthcov.hip -- the depth-to-depth second moment of Vs of many sets of rows on the FP64 matrix cores (bh_depthcov_sets).
//
// What the posterior covariance and correlation of the Vs(z) profile (bayhunter_amd/covariance.py) need beyond the
// segmented scan's means: per set S = sum_r w_r d_r d_r^T and r1 = sum_r w_r d_r over the centred rows d_r.  The result
// and the order of its sums are defined in depthcov_core.h.
//
//   depthcov_kernel   a workgroup of eight waves per (block of kDepthcovBlockRows rows of one set, group of 96 tile
//                     pairs): 32 threads per row walk 16 rows at a time with PostWalk into an LDS stage of d and
//                     e = w d, the next stage while the MFMAs of this one issue; per four rows every wave issues one
//                     v_mfma_f64_16x16x4_f64 for each of its 12 tile pairs (A: e, B: d).  The block's partial tiles, its
//                     column sums of e and its weight go to a slab.
//   depthcov_fold_kernel    one thread per (set, cell): the set's block partials added in ascending block order
//   depthcov_unpack_kernel  the tiles of the upper triangle into S [K][K], mirrored
//
// The slab holds a bounded number of blocks; a call with more takes them in runs, folding after each: the order of the
// additions is the same whatever the bound.
#include <cstring>
#include <vector>
#include "depthcov_core.h"
#include "host_common.h"
#include "stats_host.h"

namespace {

using bh::u64;
typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int SR = bh::kDepthcovStageRows, WP = bh::kDepthcovWavePairs, TILE = bh::kDepthcovTile;
constexpr int kRowThreads = bh::kDepthcovThreads / SR;         // threads that share a row's columns
constexpr size_t kSlabBytes = 256u << 20;                     // the most the slab of block partials takes,
constexpr long long kRunBlocks = 1024;                        // and the most blocks of one launch: four workgroups a CU
constexpr size_t kMaxLds = sizeof(double) * (size_t)bh::depthcov_lds_doubles(bh::depthcov_kp(BH_DEPTHCOV_MAX_K));
static_assert(kMaxLds <= bh::kLdsLimit, "the stages of the widest K fit the LDS");
static_assert(BH_DEPTHCOV_MAX_K <= bh::kDepthcovThreads, "one thread per column adds r1");

struct DepthcovArgs {
    const void *rows; long long stride; int width;
    const int *w;                      // [nrows] or NULL
    const double *extra; long long extra_stride;
    int ndep, nextra, Kp, pitch, T, npairs, nsets;
    const long long *start, *gblk;     // [nsets + 1]: rows, blocks before set z
    long long blk0;                    // the first block of this launch
    const double *dep, *center;        // [ndep], [nsets][K]
    double *slab, *r1slab;             // [blocks of the launch][npairs][TILE], [..][Kp]
    long long *totslab;                // [blocks of the launch]
    u64 *neg;
};

template <typename T>
__global__ __launch_bounds__(bh::kDepthcovThreads) void depthcov_kernel(DepthcovArgs a)
{
    extern __shared__ double lds[];                // dep [Kp] | centre [Kp] | 2 stages of d [SR][pitch], e [SR][pitch]
    __shared__ u64 s_tot;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = a.ndep + a.nextra, Kp = a.Kp, pitch = a.pitch;
    double *s_dep = lds, *s_center = lds + Kp, *stages = lds + 2 * Kp;
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
    const bool first_group = blockIdx.y == 0;      // the group that also adds r1 and the weights
    for (int c = tid; c < Kp; c += bh::kDepthcovThreads) {
        s_dep[c] = c < a.ndep ? a.dep[c] : 0.0;
        s_center[c] = c < K ? a.center[(size_t)z * K + c] : 0.0;
    }
    if (tid == 0) s_tot = 0;
    __syncthreads();

    int ti[WP], tj[WP];
    double4_t acc[WP];
    const int pbase = (int)blockIdx.y * bh::kDepthcovGroupPairs + wave * WP;
#pragma unroll
    for (int q = 0; q < WP; q++) {
        ti[q] = tj[q] = 0;                         // a pair past the last: tile (0, 0) again, never written
        if (pbase + q < a.npairs) bh::depthcov_pair(a.T, pbase + q, &ti[q], &tj[q]);
        acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
    }
    const int srow = tid / kRowThreads, seg = tid % kRowThreads;
    const T *rows = (const T *)a.rows;
    auto stage = [&](int s) {
        const int i = s * SR + srow;
        const bool have = i < nrows;
        const long long r = r0 + i;
        const int w = have ? (a.w ? a.w[r] : 1) : 0;
        if (w < 0 && seg == 0) atomicAdd(a.neg, 1ull);
        double *d = stages + (size_t)(s & 1) * (2 * SR * pitch) + srow * pitch;
        const bool in = bh::depthcov_row<T>(have ? rows + r * a.stride : nullptr, a.width, w,
                                            have && a.nextra ? a.extra + r * a.extra_stride : nullptr, a.ndep, a.nextra,
                                            s_dep, s_center, seg, Kp, kRowThreads, d, d + SR * pitch);
        if (in && seg == 0 && first_group) atomicAdd(&s_tot, (u64)w);
    };
    const int mrow = lane & 15, kq = lane >> 4;
    double r1 = 0.0;
    if (nst > 0) stage(0);
    __syncthreads();
    for (int s = 0; s < nst; s++) {
        if (s + 1 < nst) stage(s + 1);             // the other stage: free since the last barrier
        const double *dP = stages + (size_t)(s & 1) * (2 * SR * pitch), *eP = dP + SR * pitch;
        if (first_group && tid < Kp)
            for (int i = 0; i < SR; i++) r1 = r1 + eP[i * pitch + tid];
#pragma unroll
        for (int ks = 0; ks < SR / 4; ks++) {
            const int off = (ks * 4 + kq) * pitch + mrow;
#pragma unroll
            for (int q = 0; q < WP; q++)
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(eP[off + 16 * ti[q]], dP[off + 16 * tj[q]], acc[q], 0, 0, 0);
        }
        __syncthreads();
    }
    double *out = a.slab + (size_t)blockIdx.x * a.npairs * TILE;
#pragma unroll
    for (int q = 0; q < WP; q++)
        if (pbase + q < a.npairs) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) out[(size_t)(pbase + q) * TILE + reg * 64 + lane] = acc[q][reg];
        }
    if (first_group) {
        if (tid < Kp) a.r1slab[(size_t)blockIdx.x * Kp + tid] = r1;
        if (tid == 0) a.totslab[blockIdx.x] = (long long)s_tot;
    }
}

// cells of a set: npairs * TILE of S, Kp of r1, one of the weights.  Blocks [blk0, blk1) are in the slab.
__global__ void depthcov_fold_kernel(DepthcovArgs a, int z0, int nz, long long blk1, double *Sacc, double *r1acc,
                                     long long *totacc)
{
    const long long ncell = (long long)a.npairs * TILE, per = ncell + a.Kp + 1;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * nz) return;
    const int z = z0 + (int)(i / per);
    const long long c = i % per;
    const long long b0 = a.gblk[z] > a.blk0 ? a.gblk[z] : a.blk0, b1 = a.gblk[z + 1] < blk1 ? a.gblk[z + 1] : blk1;
    if (c < ncell) {
        double s = Sacc[(size_t)z * ncell + c];
        for (long long b = b0; b < b1; b++) s = s + a.slab[(size_t)(b - a.blk0) * ncell + c];
        Sacc[(size_t)z * ncell + c] = s;
    } else if (c < ncell + a.Kp) {
        const int k = (int)(c - ncell);
        double s = r1acc[(size_t)z * a.Kp + k];
        for (long long b = b0; b < b1; b++) s = s + a.r1slab[(size_t)(b - a.blk0) * a.Kp + k];
        r1acc[(size_t)z * a.Kp + k] = s;
    } else {
        long long s = totacc[z];
        for (long long b = b0; b < b1; b++) s += a.totslab[b - a.blk0];
        totacc[z] = s;
    }
}

// the upper triangle's tiles into S [nsets][K][K]; of a diagonal tile the cells with n >= m (depthcov_core.h)
__global__ void depthcov_unpack_kernel(const double *Sacc, int nsets, int K, int T, int npairs, double *S)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nsets * npairs * TILE) return;
    const int cell = (int)(i % TILE), p = (int)(i / TILE % npairs);
    const size_t z = (size_t)(i / ((long long)npairs * TILE));
    const int m = cell >> 4, n = cell & 15;
    int ti, tj;
    bh::depthcov_pair(T, p, &ti, &tj);
    const int row = 16 * ti + m, col = 16 * tj + n;
    if (row >= K || col >= K || (ti == tj && n < m)) return;
    const double v = Sacc[(z * npairs + p) * TILE + bh::depthcov_acc_slot(m, n)];
    S[(z * K + row) * K + col] = v;
    S[(z * K + col) * K + row] = v;
}

}  // namespace

extern "C" int bh_depthcov_sets(const void *rows, int fp64, long long nrows, long long stride, int width,
                                const int *weights, const double *extra, long long extra_stride, int nextra,
                                const long long *set_start, int nsets, const double *dep, int ndep, const double *center,
                                double *S, double *r1, long long *total, void *stream)
{
    if (!rows || nrows < 1) return bh::fail_arg_("bh_depthcov_sets: no rows (empty selection)");
    if (nrows > (1ll << 32)) return bh::fail_arg_("bh_depthcov_sets: more than 2^32 rows");
    if (width < 2 || stride < width) return bh::fail_arg_("bh_depthcov_sets: width >= 2 and stride >= width");
    if (ndep < 1 || !dep) return bh::fail_arg_("bh_depthcov_sets: ndep >= 1 depths");
    if (!bh::ascending(dep, ndep)) return bh::fail_arg_("bh_depthcov_sets: dep must be ascending");
    if (nextra < 0 || (nextra > 0 && (!extra || extra_stride < nextra)))
        return bh::fail_arg_("bh_depthcov_sets: extra [nrows][nextra] with extra_stride >= nextra");
    if ((long long)ndep + nextra > BH_DEPTHCOV_MAX_K) return bh::fail_arg_("bh_depthcov_sets: K = ndep + nextra above 256");
    if (nsets < 1) return bh::fail_arg_("bh_depthcov_sets: one set at least");
    if (int rc = bh::check_set_start("bh_depthcov_sets", set_start, nsets, nrows)) return rc;
    if (!center || !S || !r1 || !total) return bh::fail_arg_("bh_depthcov_sets: center, S, r1 and total");
    const int K = ndep + nextra, Kp = bh::depthcov_kp(K), T = Kp / 16, npairs = bh::depthcov_npairs(T);
    const size_t Z = (size_t)nsets, ncell = (size_t)npairs * TILE;
    std::vector<long long> gblk(Z + 1, 0);
    for (int z = 0; z < nsets; z++) gblk[z + 1] = gblk[z] + bh::depthcov_blocks(set_start[z + 1] - set_start[z]);
    const long long nblk = gblk[Z];
    if ((Z * (ncell + Kp + 1) + 255) / 256 > 0x7fffffffull)
        return bh::fail_arg_("bh_depthcov_sets: more than 2^31 - 1 workgroups in one launch");
    if (int rc = bh::require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    u64 neg = 0;                                   // before tmp: tmp drains the stream on every return, this one outlives it
    bh::CallBufs tmp(st);
    DepthcovArgs a;
    std::memset(&a, 0, sizeof(a));
    long long per_run = (long long)(kSlabBytes / (sizeof(double) * ncell));    // blocks the slab holds at a time
    per_run = per_run < 1 ? 1 : per_run > kRunBlocks ? kRunBlocks : per_run;
    const long long run = nblk < per_run ? nblk : per_run;
    long long *dstart = nullptr, *dgblk = nullptr, *dtot = nullptr;
    double *ddep = nullptr, *dcenter = nullptr, *Sacc = nullptr, *r1acc = nullptr, *dS = nullptr;
    BH_HIP(tmp.alloc(dstart, Z + 1));
    BH_HIP(tmp.alloc(dgblk, Z + 1));
    BH_HIP(tmp.alloc(ddep, (size_t)ndep));
    BH_HIP(tmp.alloc(dcenter, Z * K));
    BH_HIP(tmp.alloc(a.slab, (size_t)run * ncell));
    BH_HIP(tmp.alloc(a.r1slab, (size_t)run * Kp));
    BH_HIP(tmp.alloc(a.totslab, (size_t)run));
    BH_HIP(tmp.alloc(a.neg, 1));
    BH_HIP(tmp.alloc(Sacc, Z * ncell));
    BH_HIP(tmp.alloc(r1acc, Z * Kp));
    BH_HIP(tmp.alloc(dtot, Z));
    BH_HIP(tmp.alloc(dS, Z * K * K));
    BH_HIP(hipMemcpyAsync(dstart, set_start, sizeof(long long) * (Z + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dgblk, gblk.data(), sizeof(long long) * (Z + 1), hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(ddep, dep, sizeof(double) * ndep, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemcpyAsync(dcenter, center, sizeof(double) * Z * K, hipMemcpyHostToDevice, st));
    BH_HIP(hipMemsetAsync(a.neg, 0, sizeof(u64), st));
    BH_HIP(hipMemsetAsync(Sacc, 0, sizeof(double) * Z * ncell, st));
    BH_HIP(hipMemsetAsync(r1acc, 0, sizeof(double) * Z * Kp, st));
    BH_HIP(hipMemsetAsync(dtot, 0, sizeof(long long) * Z, st));
    a.rows = rows; a.stride = stride; a.width = width;
    a.w = weights;
    a.extra = extra; a.extra_stride = extra_stride;
    a.ndep = ndep; a.nextra = nextra; a.Kp = Kp; a.pitch = bh::depthcov_pitch(Kp); a.T = T; a.npairs = npairs;
    a.nsets = nsets;
    a.start = dstart; a.gblk = dgblk;
    a.dep = ddep; a.center = dcenter;
    const size_t dyn = sizeof(double) * (size_t)bh::depthcov_lds_doubles(Kp);
    const void *fn = fp64 ? (const void *)depthcov_kernel<double> : (const void *)depthcov_kernel<float>;
    BH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
    const unsigned groups = (unsigned)((npairs + bh::kDepthcovGroupPairs - 1) / bh::kDepthcovGroupPairs);
    int z0 = 0;                                    // the first set with a block at or after blk0
    for (long long b0 = 0; b0 < nblk; b0 += run) {
        const long long b1 = b0 + run < nblk ? b0 + run : nblk;
        a.blk0 = b0;
        const dim3 grid((unsigned)(b1 - b0), groups);
        if (fp64) hipLaunchKernelGGL(depthcov_kernel<double>, grid, dim3(bh::kDepthcovThreads), dyn, st, a);
        else hipLaunchKernelGGL(depthcov_kernel<float>, grid, dim3(bh::kDepthcovThreads), dyn, st, a);
        BH_HIP(hipGetLastError());
        while (gblk[z0 + 1] <= b0) z0++;
        int z1 = z0;                               // the last set with a block before b1
        while (z1 + 1 < nsets && gblk[z1 + 1] < b1) z1++;
        const long long cells = (long long)(z1 - z0 + 1) * (long long)(ncell + Kp + 1);
        hipLaunchKernelGGL(depthcov_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a, z0,
                           z1 - z0 + 1, b1, Sacc, r1acc, dtot);
        BH_HIP(hipGetLastError());
    }
    BH_HIP(hipMemsetAsync(dS, 0, sizeof(double) * Z * K * K, st));
    hipLaunchKernelGGL(depthcov_unpack_kernel, dim3((unsigned)((Z * ncell + 255) / 256)), dim3(256), 0, st,
                       (const double *)Sacc, nsets, K, T, npairs, dS);
    BH_HIP(hipGetLastError());
    std::vector<double> hr1(Z * Kp);
    BH_HIP(hipMemcpyAsync(&neg, a.neg, sizeof(u64), hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(S, dS, sizeof(double) * Z * K * K, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(hr1.data(), r1acc, sizeof(double) * Z * Kp, hipMemcpyDeviceToHost, st));
    BH_HIP(hipMemcpyAsync(total, dtot, sizeof(long long) * Z, hipMemcpyDeviceToHost, st));
    BH_HIP(hipStreamSynchronize(st));
    if (neg) return bh::fail_arg_("bh_depthcov_sets: negative weight");
    for (size_t z = 0; z < Z; z++)
        for (int k = 0; k < K; k++) r1[z * K + k] = hr1[z * Kp + k];
    return BH_OK;
}
