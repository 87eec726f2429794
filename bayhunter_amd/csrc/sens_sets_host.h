// sens_sets_host.h -- what the two depth-binned sensitivity reductions share around their main kernels (sens_sets.hip:
// dc/dm at periods; rf_sens_sets.hip: dRF(t)/dm at a trace's samples): the sets of a handle in a global row numbering,
// where a call may cut them, the list of blocks a call's rows make (sens_sets_core.h: the order of the sums), the checks
// of what both `create` and both `add` calls take alike, and the handle itself (SensSetsHandle): its device buffers, the
// fold and init kernels, the chunk loop of an add and the finish.  A file keeps its main kernel, that kernel's arguments
// and launch, and the checks of what only it takes.
#pragma once
#include <cmath>
#include <vector>
#include "sens_sets_core.h"
#include "host_common.h"
#include "stats_host.h"

namespace bh {

constexpr size_t kSensSetsSlabBytes = 64u << 20;    // the most the slab of block partials takes

struct SensSetRows {
    int nsets = 0;
    std::vector<long long> start;                  // [nsets + 1]
    long long next = 0;                            // the row the next add begins with

    long long total_rows() const { return start[nsets]; }
    // the set row r lies in (r < total_rows()): the last set that begins at or before r
    int set_of(long long r) const
    {
        int lo = 0, hi = nsets;
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (start[mid] <= r) lo = mid;
            else hi = mid;
        }
        return lo;
    }
    // may a call begin or end at row r: at a set's first row, at the end, or a whole number of blocks into a set
    bool cut_ok(long long r) const
    {
        if (r == 0 || r == total_rows()) return true;
        return (r - start[set_of(r)]) % kSensSetsBlockRows == 0;
    }
    // the blocks of all sets together
    long long blocks() const
    {
        long long n = 0;
        for (int z = 0; z < nsets; z++) n += (start[z + 1] - start[z] + kSensSetsBlockRows - 1) / kSensSetsBlockRows;
        return n;
    }
    // the blocks of rows row0 .. row0 + B - 1 (cut_ok at both ends): (set, first row within the call, rows)
    void call_blocks(long long row0, int B, std::vector<int3> &blocks) const
    {
        const long long end = row0 + B;
        for (int z = set_of(row0); z < nsets && start[z] < end; z++) {
            const long long a = start[z] > row0 ? start[z] : row0, b = start[z + 1] < end ? start[z + 1] : end;
            for (long long r = a; r < b; r += kSensSetsBlockRows)
                blocks.push_back(make_int3(z, (int)(r - row0), (int)(b - r < kSensSetsBlockRows ? b - r : kSensSetsBlockRows)));
        }
    }
    // blocks a slab of kSensSetsSlabBytes holds at `nitems` partials a block: one at least, no more than there are
    size_t slab_blocks(size_t nitems) const
    {
        const size_t fit = kSensSetsSlabBytes / (nitems * sizeof(SensSetsAcc));
        size_t cap = fit < 1 ? 1 : fit;
        const long long n = blocks();
        if ((long long)cap > n) cap = n < 1 ? 1 : (size_t)n;
        return cap;
    }
};

// create's handle and sets
inline int sens_sets_check_sets(const char *who, void **handle, const long long *set_start, int nsets)
{
    if (!handle) return fail_who(who, "NULL handle");
    *handle = nullptr;
    if (nsets < 1 || nsets > BH_PAIRS_MAX_SETS) return fail_who(who, "1 to 65535 sets");
    if (!set_start || set_start[0] != 0) return fail_who(who, "set_start must begin at 0");
    return check_set_start(who, set_start, nsets, set_start[nsets]);
}

// create's depth edges, kind and drho_dvp
inline int sens_sets_check_grid(const char *who, const double *edges, int nedges, int kind, double drho_dvp)
{
    if (!edges || nedges < 2 || nedges > BH_SENS_SETS_MAX_BINS + 1) return fail_who(who, "depth edges: 2 to 1025");
    if (!ascending(edges, nedges) || !std::isfinite(edges[0]) || !std::isfinite(edges[nedges - 1]))
        return fail_who(who, "depth edges must be finite and ascending");
    if (!sens_sets_kind_ok(kind)) return fail_who(who, "kind: BH_SENS_KIND_VP, _VS, _RHO or _VS_TOTAL");
    if (!std::isfinite(drho_dvp)) return fail_who(who, "drho_dvp must be finite");
    return BH_OK;
}

// what add checks of the rows before it looks at the arrays (NULL: nothing is wrong)
inline const char *sens_sets_rows_fault(const SensSetRows &rows, long long row0, int B)
{
    if (row0 != rows.next) return "the rows must arrive in ascending order without a gap";
    if (row0 + B > rows.total_rows()) return "more rows than set_start holds";
    return nullptr;
}

constexpr const char *kSensSetsCutFault = "a call may begin or end inside a set only at a multiple of "
                                          "BH_SENS_SETS_BLOCK_ROWS rows from the set's first row";

// ---- the device side of a handle ------------------------------------------------------------------------------------
// (static: a plain kernel in a header is compiled into every file that includes it; both files launch both)

// A chunk's partials into their sets' sums, in block order.  A block carries nitems partials and nw (total, excluded)
// weight pairs -- one per period (sens_sets.hip), one (rf_sens_sets.hip).  Thread t < nitems: item t; the next nw
// threads: weight pair t - nitems.
static __global__ void sens_sets_fold_kernel(const int3 *blocks, int nblocks, int nitems, int nw, const SensSetsAcc *slab,
                                             const long long *wslab, SensSetsAcc *acc, long long *wacc)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nitems) {
        int z = -1;
        SensSetsAcc cur;
        sens_sets_acc_init(cur);
        for (int b = 0; b < nblocks; b++) {
            const int zb = blocks[b].x;
            if (zb != z) {
                if (z >= 0) acc[(size_t)z * nitems + t] = cur;
                z = zb;
                cur = acc[(size_t)z * nitems + t];
            }
            sens_sets_acc_fold(cur, slab[(size_t)b * nitems + t]);
        }
        if (z >= 0) acc[(size_t)z * nitems + t] = cur;
    } else if (t < nitems + nw) {
        const int p = t - nitems;
        for (int b = 0; b < nblocks; b++) {
            long long *out = wacc + ((size_t)blocks[b].x * nw + p) * 2;
            out[0] += wslab[((size_t)b * nw + p) * 2];
            out[1] += wslab[((size_t)b * nw + p) * 2 + 1];
        }
    }
}

static __global__ void sens_sets_init_kernel(SensSetsAcc *acc, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sens_sets_acc_init(acc[i]);
}

// What a handle of either reduction is besides its main kernel: the sets, the grid, and on the device the slab of block
// partials, the sets' sums and the count of negative weights.  A file sets nsets .. st, rows and edges in its create
// and derives its own handle from this one.
struct SensSetsHandle {
    int nsets = 0, nb = 0, kind = 0;
    int nw = 1;                                    // (total, excluded) weight pairs a block carries
    size_t nitems = 0;                             // partials a block carries: nitems / nw per weight pair
    double drho = 0.0;
    hipStream_t st = nullptr;
    SensSetRows rows;                              // the sets, and the row the next add begins with
    std::vector<double> edges;                     // [nb + 1]
    bool ready = false;                            // the device buffers are there
    size_t cap = 1;                                // blocks the slab holds
    DevBufs bufs;
    double *dedges = nullptr;
    int3 *dblocks = nullptr;
    SensSetsAcc *slab = nullptr, *acc = nullptr;   // [cap][nitems], [nsets][nitems]
    long long *wslab = nullptr, *wacc = nullptr;   // [cap][nw][2], [nsets][nw][2]
    u64 *neg = nullptr;                            // rows with a negative weight

    // the sets, the grid and the stream of create's arguments (checked)
    void init(const long long *set_start, int nsets_, const double *e, int nedges, int kind_, double drho_dvp, void *stream)
    {
        nsets = nsets_;
        nb = nedges - 1;
        kind = kind_;
        drho = drho_dvp;
        st = (hipStream_t)stream;
        rows.nsets = nsets_;
        rows.start.assign(set_start, set_start + nsets_ + 1);
        edges.assign(e, e + nedges);
    }
    // once: the device, the buffers, the accumulators at their start
    int make_ready()
    {
        if (ready) return BH_OK;
        if (int rc = require_device()) return rc;
        const size_t cells = (size_t)nsets * nitems;
        cap = rows.slab_blocks(nitems);
        BH_HIP(bufs.alloc(dedges, edges.size()));
        BH_HIP(bufs.alloc(dblocks, cap));
        BH_HIP(bufs.alloc(slab, cap * nitems));
        BH_HIP(bufs.alloc(wslab, cap * nw * 2));
        BH_HIP(bufs.alloc(acc, cells));
        BH_HIP(bufs.alloc(wacc, (size_t)nsets * nw * 2));
        BH_HIP(bufs.alloc(neg, 1));
        BH_HIP(hipMemcpyAsync(dedges, edges.data(), sizeof(double) * edges.size(), hipMemcpyHostToDevice, st));
        BH_HIP(hipMemsetAsync(wacc, 0, sizeof(long long) * (size_t)nsets * nw * 2, st));
        BH_HIP(hipMemsetAsync(neg, 0, sizeof(u64), st));
        hipLaunchKernelGGL(sens_sets_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, acc, cells);
        BH_HIP(hipGetLastError());
        ready = true;
        return BH_OK;
    }
    // What both adds check alike, in the order they report it; `own` is the fault among the file's own arguments (NULL:
    // none), reported after a NULL pointer and before the cut.  BH_OK with B == 0: there is nothing to add.
    int check_add(const char *who, long long row0, int B, int Lmax, int model_stride, const int *nlay, const double *hthk,
                  const double *q, int q_stride, const double *K, const char *own) const
    {
        if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail_who(who, "B/Lmax out of range");
        if (model_stride < Lmax) return fail_who(who, "model_stride < Lmax");
        if (const char *fault = sens_sets_rows_fault(rows, row0, B)) return fail_who(who, fault);
        if (B == 0) return BH_OK;
        if (kind == BH_SENS_KIND_VS_TOTAL && !q) return fail_who(who, "BH_SENS_KIND_VS_TOTAL needs q");
        if (q && q_stride < Lmax) return fail_who(who, "q_stride < Lmax");
        if (!nlay || !hthk || !K) return fail_who(who, "NULL pointer");
        if (own) return fail_who(who, own);
        if (!rows.cut_ok(row0) || !rows.cut_ok(row0 + B)) return fail_who(who, kSensSetsCutFault);
        return BH_OK;
    }
    // Rows row0 .. row0 + B - 1 (checked; the handle ready): their blocks in chunks of at most `cap`, each through the
    // file's main kernel -- launch(nblocks) reads dblocks and fills slab and wslab -- and folded before the next is
    // launched.  The call's arrays are free when it returns, and a negative weight is reported by the call that brought it.
    template <typename Launch>
    int add(const char *who, long long row0, int B, Launch launch)
    {
        std::vector<int3> blocks;
        CallBufs drain(st);                         // (owns nothing: an early return waits for the copies of `blocks`)
        rows.call_blocks(row0, B, blocks);
        const unsigned fold = (unsigned)((nitems + nw + 255) / 256);
        for (size_t b0 = 0; b0 < blocks.size(); b0 += cap) {
            const size_t n = blocks.size() - b0 < cap ? blocks.size() - b0 : cap;
            BH_HIP(hipMemcpyAsync(dblocks, blocks.data() + b0, sizeof(int3) * n, hipMemcpyHostToDevice, st));
            launch((unsigned)n);
            BH_HIP(hipGetLastError());
            hipLaunchKernelGGL(sens_sets_fold_kernel, dim3(fold), dim3(256), 0, st, (const int3 *)dblocks, (int)n, (int)nitems,
                               nw, (const SensSetsAcc *)slab, (const long long *)wslab, acc, wacc);
            BH_HIP(hipGetLastError());
        }
        u64 bad = 0;
        BH_HIP(hipMemcpyAsync(&bad, neg, sizeof(u64), hipMemcpyDeviceToHost, st));
        BH_HIP(hipStreamSynchronize(st));
        rows.next = row0 + B;
        if (bad) return fail_who(who, "negative weight");
        return BH_OK;
    }
    // The sums to the caller's arrays (any may be NULL): total, excluded [nsets][nw]; s1 .. vmax [nsets][nitems].  A
    // weight pair without a row that counts: sums 0, min / max NaN.  A handle that was never made ready has no row and
    // finishes without a device.
    int finish(const char *who, long long *total, long long *excluded, double *s1, double *s2, double *vmin, double *vmax)
    {
        if (rows.next != rows.total_rows()) return fail_who(who, "not all rows of set_start were added");
        const size_t pairs = (size_t)nsets * nw, per = nitems / nw;
        std::vector<SensSetsAcc> a;
        std::vector<long long> w(pairs * 2, 0);
        if (ready) {
            u64 bad = 0;
            a.resize(pairs * per);
            BH_HIP(hipMemcpyAsync(a.data(), acc, sizeof(SensSetsAcc) * a.size(), hipMemcpyDeviceToHost, st));
            BH_HIP(hipMemcpyAsync(w.data(), wacc, sizeof(long long) * w.size(), hipMemcpyDeviceToHost, st));
            BH_HIP(hipMemcpyAsync(&bad, neg, sizeof(u64), hipMemcpyDeviceToHost, st));
            BH_HIP(hipStreamSynchronize(st));
            if (bad) return fail_who(who, "negative weight");
        }
        const double nan = std::nan("");
        for (size_t zp = 0; zp < pairs; zp++) {
            const bool any = w[2 * zp] > 0;
            if (total) total[zp] = w[2 * zp];
            if (excluded) excluded[zp] = w[2 * zp + 1];
            for (size_t i = zp * per; i < (zp + 1) * per; i++) {
                if (s1) s1[i] = any ? a[i].s1 : 0.0;
                if (s2) s2[i] = any ? a[i].s2 : 0.0;
                if (vmin) vmin[i] = any ? a[i].vmin : nan;
                if (vmax) vmax[i] = any ? a[i].vmax : nan;
            }
        }
        return BH_OK;
    }
    ~SensSetsHandle()
    {
        if (ready) (void)hipStreamSynchronize(st);  // (a handle that never saw a row never saw the device)
    }
};

}  // namespace bh
