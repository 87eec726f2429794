// stats_host.h -- the host scaffolding of the weighted column reductions (posterior.hip, datafits.hip).
//
// Both reduce n columns (depths there, samples of the modelled data here) over rows with integer weights in a
// scan pass and a finish pass: min / max over order-preserving keys, Σ through a per-block slab that one thread
// per column adds in block order, histograms over host-made edges, order statistics by radix select
// (stats_core.h).  The rows come in contiguous sets (one block = one set); a handle over one set of rows is the
// same handle with a single set.  Only the way a block reads a value differs, and that stays in the files; what
// surrounds it is here: the owner of device buffers, the fill and slab kernels, the select's device side, the part
// of a handle that carries a scan over to its finish (SetStats), and the set_start check every segmented entry
// point makes (bh_moho_sets too).
// (Errors and the device check: host_common.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <vector>
#include "host_common.h"
#include "stats_core.h"

namespace bh {

typedef unsigned long long u64;

// owns what it allocates: a handle's buffers for the handle's life, a call's for the call
class DevBufs {
    std::vector<void *> bufs_;
public:
    DevBufs() = default;
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    ~DevBufs() { for (void *b : bufs_) (void)hipFree(b); }
    template <typename T>
    hipError_t alloc(T *&ptr, size_t count)
    {
        bufs_.push_back(nullptr);
        hipError_t e = hipMalloc(&bufs_.back(), sizeof(T) * count);
        ptr = (T *)bufs_.back();
        return e;
    }
};

// a call's buffers whose kernels may still be queued when the call returns early: the stream is drained before they go
struct CallBufs : DevBufs {
    hipStream_t st;
    explicit CallBufs(hipStream_t s) : st(s) {}
    ~CallBufs() { (void)hipStreamSynchronize(st); }
};

static __global__ void stats_fill_kernel(u64 *p, int n, u64 v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

inline bool ascending(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!(v[i] == v[i]) || (i && !(v[i - 1] < v[i]))) return false;
    return true;
}

// a device histogram into the caller's: synchronises
inline int read_hist(const u64 *dhist, size_t count, long long *hist, hipStream_t st)
{
    std::vector<u64> h(count);
    BH_HIP(hipMemcpyAsync(h.data(), dhist, sizeof(u64) * count, hipMemcpyDeviceToHost, st));
    BH_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < count; i++) hist[i] = (long long)h[i];
    return BH_OK;
}

// The select with its device side: what a pass's kernel reads (the groups) and what it adds to (digits[slots][256]).
// A pass is begin_pass, the caller's kernel at digit `shift`, end_pass; until done().
struct DeviceSelect : RadixSelect {
    int *dgbase = nullptr, *dngroups = nullptr;
    u64 *dgpfx = nullptr, *ddigits = nullptr;
    std::vector<uint64_t> dig;
    using RadixSelect::RadixSelect;

    int alloc(DevBufs &bufs)
    {
        BH_HIP(bufs.alloc(dgbase, ncols));
        BH_HIP(bufs.alloc(dngroups, ncols));
        BH_HIP(bufs.alloc(dgpfx, pfx.size()));
        BH_HIP(bufs.alloc(ddigits, 256 * pfx.size()));
        return BH_OK;
    }
    int begin_pass(hipStream_t st)
    {
        plan();
        BH_HIP(hipMemcpyAsync(dgbase, gbase.data(), sizeof(int) * ncols, hipMemcpyHostToDevice, st));
        BH_HIP(hipMemcpyAsync(dngroups, ngroups.data(), sizeof(int) * ncols, hipMemcpyHostToDevice, st));
        BH_HIP(hipMemcpyAsync(dgpfx, gpfx.data(), sizeof(u64) * slots, hipMemcpyHostToDevice, st));
        BH_HIP(hipMemsetAsync(ddigits, 0, sizeof(u64) * 256 * (size_t)slots, st));
        return BH_OK;
    }
    int end_pass(hipStream_t st)             // synchronises
    {
        dig.resize((size_t)slots * 256);
        BH_HIP(hipMemcpyAsync(dig.data(), ddigits, sizeof(u64) * dig.size(), hipMemcpyDeviceToHost, st));
        BH_HIP(hipStreamSynchronize(st));
        advance(dig.data());
        return BH_OK;
    }
};

// what is wrong with a scan's counts, in the words every entry point reports it (NULL: nothing)
// (bayhunter_amd/moho.py recognises "empty selection" in a bh_datafits_scan error as "no row has a Moho": keep the words)
inline const char *scan_fault(u64 included, u64 negative)
{
    return negative ? "negative weight"
           : included == 0 ? "empty selection (no included row with a positive weight)"
           : included > (1ull << 53) ? "weight total above 2^53" : nullptr;
}

// an argument error of the entry point `who`: "<who>: <what>" (static: the library exports no symbol for it)
static inline int fail_who(const char *who, const char *what)
{
    return bh::fail_arg_((std::string(who) + ": " + what).c_str());
}

// ---- the rows come in contiguous segments: set z is rows start[z] .. start[z + 1] -----------------------------------

// Σ over a set's blocks in block order: one thread per (set, column); set z owns slab rows goff[z] .. goff[z + 1]
// (a template, and SetStats below one on the file's blocks_of: a plain kernel in a header is compiled into every file
// that includes it, and moho.hip takes from here the buffers and the set_start check only)
template <typename T>
static __global__ void stats_sets_reduce_kernel(const T *slab, const long long *goff, int nsets, int n, T *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nsets * n) return;
    const int z = (int)(i / n), c = (int)(i % n);
    const int G = (int)(goff[z + 1] - goff[z]);
    const T *sl = slab + (size_t)goff[z] * n;
    T s = 0.0;
    for (int g = 0; g < G; g++) s = s + sl[(size_t)g * n + c];
    out[i] = s;
}

// the segments of an entry point `who`: from row 0 to row nrows, ascending (a set may be empty)
inline int check_set_start(const char *who, const long long *set_start, int nsets, long long nrows)
{
    if (!set_start || set_start[0] != 0 || set_start[nsets] != nrows)
        return fail_who(who, "set_start must begin at 0 and end at nrows");
    for (int z = 0; z < nsets; z++)
        if (set_start[z] > set_start[z + 1]) return fail_who(who, "set_start must be ascending");
    return BH_OK;
}

// why a set of a segmented scan has no statistics, in scan_fault's words ("": it has)
static_assert(BH_POSTERIOR_SET_OK == BH_DATAFITS_SET_OK && BH_POSTERIOR_SET_EMPTY == BH_DATAFITS_SET_EMPTY &&
              BH_POSTERIOR_SET_OVERFLOW == BH_DATAFITS_SET_OVERFLOW, "one status per set for both segmented reductions");
inline const char *set_status_text(int status)
{
    return status == BH_POSTERIOR_SET_EMPTY ? scan_fault(0, 0)
           : status == BH_POSTERIOR_SET_OVERFLOW ? scan_fault(~0ull, 0) : "";
}

// The part of a handle both reductions share: n columns of nsets sets, and what a scan leaves for the finish.  A
// block belongs to one set and is block x of the G(z) blocks of the set -- a function of the set's row count only (the
// file's own blocks_of), so that the slab order of a set is fixed whatever its offset and its neighbours; the sets'
// slab rows lie one after the other, so a pass takes every set in one launch and one reduction.
enum { SET_SKIP = 1 };                 // skip[z] & SET_SKIP: the finish leaves set z out (the other bits are the file's)
template <int (*BlocksOf)(long long)>
struct SetStats {
    int n = 0, nsets = 0, Gmax = 1, scanned = 0;
    hipStream_t st = nullptr;
    std::vector<long long> start, goff;          // [nsets + 1] rows, slab rows before set z
    std::vector<u64> total;                      // [nsets] weight totals of the scan
    std::vector<int> status, skip;               // [nsets] BH_*_SET_* of the scan; of the finish
    DevBufs bufs;
    long long *dstart = nullptr, *dgoff = nullptr;
    int *dskip = nullptr;
    double *slab = nullptr, *red = nullptr, *dmean = nullptr;    // [goff[nsets]][n], [nsets][n], [nsets][n]
    u64 *kmin = nullptr, *kmax = nullptr;                        // [nsets][n]

    size_t cols() const { return (size_t)nsets * n; }
    int G(int z) const { return (int)(goff[z + 1] - goff[z]); }
    // the grid's x extent for sets [first, first + nc): the blocks of the largest of them
    int chunk_blocks(int first, int nc) const
    {
        int g = 1;
        for (int z = first; z < first + nc; z++) g = G(z) > g ? G(z) : g;
        return g;
    }
    // n, nsets and st are set: the segments, their slab offsets by the file's blocks_of, and the buffers
    int alloc_sets(const long long *set_start)
    {
        start.assign(set_start, set_start + nsets + 1);
        goff.assign((size_t)nsets + 1, 0);
        Gmax = set_slab_offsets(start.data(), nsets, BlocksOf, goff.data());
        total.assign(nsets, 0);
        status.assign(nsets, BH_POSTERIOR_SET_EMPTY);
        skip.assign(nsets, 0);
        BH_HIP(bufs.alloc(dstart, (size_t)nsets + 1));
        BH_HIP(bufs.alloc(dgoff, (size_t)nsets + 1));
        BH_HIP(bufs.alloc(dskip, nsets));
        BH_HIP(bufs.alloc(slab, (size_t)goff[nsets] * n));
        BH_HIP(bufs.alloc(red, cols()));
        BH_HIP(bufs.alloc(dmean, cols()));
        BH_HIP(bufs.alloc(kmin, cols()));
        BH_HIP(bufs.alloc(kmax, cols()));
        BH_HIP(hipMemcpyAsync(dstart, start.data(), sizeof(long long) * ((size_t)nsets + 1), hipMemcpyHostToDevice, st));
        BH_HIP(hipMemcpyAsync(dgoff, goff.data(), sizeof(long long) * ((size_t)nsets + 1), hipMemcpyHostToDevice, st));
        return BH_OK;
    }
    // a scan starts: whatever an earlier one left is void until this one has succeeded; the file's counters are 0
    int begin_scan(u64 *cnt, size_t ncnt)
    {
        scanned = 0;
        const int m = (int)cols();
        hipLaunchKernelGGL(stats_fill_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, kmin, m, ~0ull);
        hipLaunchKernelGGL(stats_fill_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, kmax, m, 0ull);
        BH_HIP(hipGetLastError());
        BH_HIP(hipMemsetAsync(cnt, 0, sizeof(u64) * ncnt, st));
        return BH_OK;
    }
    // the slab of the pass just launched, added up per set: synchronises
    int reduce_slab(std::vector<double> &out)
    {
        hipLaunchKernelGGL(stats_sets_reduce_kernel<double>, dim3((unsigned)((cols() + 255) / 256)), dim3(256), 0, st,
                           (const double *)slab, (const long long *)dgoff, nsets, n, red);
        BH_HIP(hipGetLastError());
        out.assign(cols(), 0.0);
        BH_HIP(hipMemcpyAsync(out.data(), red, sizeof(double) * cols(), hipMemcpyDeviceToHost, st));
        BH_HIP(hipStreamSynchronize(st));
        return BH_OK;
    }
    // a scan ends, with each set's counts and reduce_slab's Σ w·v on the host: a negative weight anywhere is an error
    // (`who` names the entry point); else every set its total and status, a live set (status 0) its mean -- to the
    // device for the finish -- and min / max back from their keys, any other set NaN
    int end_scan(const char *who, const std::vector<u64> &included, const std::vector<u64> &negative,
                 const std::vector<double> &sum, long long *tot, int *stat, double *vmin, double *vmax, double *mean)
    {
        for (int z = 0; z < nsets; z++)
            if (negative[z]) return fail_who(who, scan_fault(included[z], negative[z]));
        std::vector<u64> kmn(cols()), kmx(cols());
        BH_HIP(hipMemcpyAsync(kmn.data(), kmin, sizeof(u64) * cols(), hipMemcpyDeviceToHost, st));
        BH_HIP(hipMemcpyAsync(kmx.data(), kmax, sizeof(u64) * cols(), hipMemcpyDeviceToHost, st));
        std::vector<double> mu(cols());
        const double nan = std::nan("");
        for (int z = 0; z < nsets; z++) {
            total[z] = included[z];
            status[z] = included[z] == 0 ? BH_POSTERIOR_SET_EMPTY
                        : included[z] > (1ull << 53) ? BH_POSTERIOR_SET_OVERFLOW : BH_POSTERIOR_SET_OK;
            stat[z] = status[z];
            if (tot) tot[z] = (long long)included[z];
            for (int c = 0; c < n; c++)
                mu[(size_t)z * n + c] = status[z] == BH_POSTERIOR_SET_OK ? sum[(size_t)z * n + c] / (double)included[z] : nan;
        }
        BH_HIP(hipMemcpyAsync(dmean, mu.data(), sizeof(double) * cols(), hipMemcpyHostToDevice, st));
        BH_HIP(hipStreamSynchronize(st));
        for (int z = 0; z < nsets; z++)
            for (int c = 0; c < n; c++) {
                const size_t i = (size_t)z * n + c;
                const bool live = status[z] == BH_POSTERIOR_SET_OK;
                if (vmin) vmin[i] = live ? bh::post_unkey64(kmn[i]) : nan;
                if (vmax) vmax[i] = live ? bh::post_unkey64(kmx[i]) : nan;
                if (mean) mean[i] = mu[i];
            }
        scanned = 1;
        return BH_OK;
    }
    // the finish's skip flags to the device, before its first launch
    int upload_skip()
    {
        BH_HIP(hipMemcpyAsync(dskip, skip.data(), sizeof(int) * nsets, hipMemcpyHostToDevice, st));
        return BH_OK;
    }
    // the finish pass's slab of Σ w·(v - mean)² -> population std, NaN for a set left out: synchronises
    int read_stdev(double *stdev)
    {
        std::vector<double> sq;
        int rc = reduce_slab(sq);
        if (rc) return rc;
        for (int z = 0; z < nsets; z++)
            for (int c = 0; c < n; c++) {
                const size_t i = (size_t)z * n + c;
                stdev[i] = (skip[z] & SET_SKIP) ? std::nan("") : std::sqrt(sq[i] / (double)total[z]);
            }
        return BH_OK;
    }
};

}  // namespace bh
