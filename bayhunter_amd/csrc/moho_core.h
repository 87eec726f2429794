// moho_core.h -- per-row arithmetic of the Moho / crustal-velocity posterior (moho.hip).
//
// A row is a model in the reference's layout [vs(n), z_vnoi(n), NaN...] (src/Models.py:16-24) in float32 or
// float64.  What PlotFromStorage.plot_moho_crustvel_tradeoff derives from it (src/Plotting.py:766-798), with
// h from Model.get_vp_vs_h (Models.py:40-52):
//
//   z_disc = (z[:n-1] + z[1:n]) / 2.            in the row's dtype: a float32 sum and a float32 half
//   h      = z_disc - [0, z_disc[:-1]], 0       fp64 (the list [0] makes the subtrahend int64 -> float64)
//   ifaces = cumsum(h)                          fp64, sequential
//   Moho   = the first i in 0 .. n-2 with  zlo < ifaces[i] < zhi  and  vs[i+1] > mohovs   (strict; the velocity
//            compared in the row's dtype, so mohovs is rounded to it first)
//   moho = ifaces[i],  vs_crust = sum(vs[:i+1] * h[:i+1]) / ifaces[i],  vs_last = vs[i],
//   vs_jump = vs[i+1] - vs[i]                   a difference in the row's dtype
//
// np.sum over m = i + 1 fp64 products: for m < 8 from 0 left to right; for m >= 8 (m <= 128 always: at most
// BH_MAX_LAYERS layers) eight accumulators r[j] = a[j], r[j] += a[8 b + j] over the complete blocks of eight,
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), and then the m % 8 remaining terms one after the other.
//
// PostWalk (posterior_core.h) forms z_disc in double, which is right for np.interp's knots there and wrong here
// for float32 rows; this walk follows its shape -- it reads vs / z from the row as it crosses an interface and
// keeps no layer list -- with the interface rounded as above.  The eight accumulators and the eight pending
// products of the current block are indexed by the unrolled inner loop only, so they stay in registers.
// Compiled with g++ under BH_HOSTSIM by tests/hostsim/moho_sim.cpp (test infrastructure only).
#pragma once
#include "bh_common.h"
#include "posterior_core.h"

namespace bh {

BH_HD double moho_tree8(const double *r)
{
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// out[4] = (moho, vs_crust, vs_last, vs_jump) of a row, all NaN when it has no Moho; -> 1 with a Moho.
// A Moho whose derived values hold a NaN (an interface at depth 0 with nothing above it, infinite velocities)
// counts as none: the four values are NaN together or not at all.
template <typename T>
BH_HD int moho_row(const T *row, int width, double zlo, double zhi, double mohovs, double *out)
{
    const double nan = __builtin_nan("");
    out[0] = out[1] = out[2] = out[3] = nan;
    const int count = post_row_count(row, width);
    const int n = count / 2;
    if (n < 2) return 0;
    const int zoff = count - n;                     // model[-n:] of split_modelparams
    const T vlim = (T)mohovs;
    double r[8], p[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = p[j] = 0.0;
    double D = 0.0, prev = 0.0;                     // ifaces[k - 1], z_disc[k - 1] widened
    double seq = 0.0;                               // np.sum of the first k + 1 products
    T znext = row[zoff];
    T vsk = row[0];
    for (int b = 0; 8 * b < n - 1; b++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int k = 8 * b + j;
            if (k < n - 1) {
                const T zk = znext;
                znext = row[zoff + k + 1];
                const T zd = (T)((T)(zk + znext) / (T)2);
                const double h = (double)zd - prev;
                prev = (double)zd;
                D = k == 0 ? h : D + h;             // cumsum copies its first element
                p[j] = (double)vsk * h;
                if (j == 7) {                       // a block of eight is complete: the sum is the tree alone
#pragma unroll
                    for (int i = 0; i < 8; i++) r[i] = b == 0 ? p[i] : r[i] + p[i];
                    seq = 0.0 + moho_tree8(r);      // the reduction adds numpy's tree to its identity 0: -0 -> +0
                } else {                            // from 0 (first block) or from the tree, term after term
                    seq = seq + p[j];
                }
                const T vnext = row[k + 1];
                if (D > zlo && D < zhi && vnext > vlim) {
                    const double crust = seq / D;
                    const double last = (double)vsk;
                    const double jump = (double)(T)(vnext - vsk);
                    if (!(D == D) || !(crust == crust) || !(last == last) || !(jump == jump)) return 0;
                    out[0] = D;
                    out[1] = crust;
                    out[2] = last;
                    out[3] = jump;
                    return 1;
                }
                vsk = vnext;
            }
        }
    }
    return 0;
}

}  // namespace bh
