// sens_sets_host.h -- the host bookkeeping the two depth-binned sensitivity reductions share (sens_sets.hip: dc/dm at
// periods; rf_sens_sets.hip: dRF(t)/dm at a trace's samples): the sets of a handle in a global row numbering, where a
// call may cut them, the list of blocks a call's rows make (sens_sets_core.h: the order of the sums), and the checks of
// what both `create` calls take alike.
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

}  // namespace bh
