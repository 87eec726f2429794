// posterior_core.h -- per-row arithmetic of the velocity-depth posterior (posterior.hip).
//
// A row is a model in the reference's layout [vs(n), z_vnoi(n), NaN...] (src/Models.py:16-24) in
// float32 or float64.  Its Vs on an ascending depth grid is what Model.get_interpmodel returns
// (Models.py:55-70,94-113): interfaces z_disc = (z[i] + z[i+1]) / 2, thicknesses h = z_disc - [0,
// z_disc[:-1]], depths the sequential fp64 cumsum of h, and np.interp over the step knots, which puts
// a point exactly on an interface into the deeper layer, points below the last interface into the
// half-space and points above 0 into the top layer.  The value is always one of the stored Vs values.
//
// The walk never holds the layer list in an array: it reads vs / z from the row as it crosses an
// interface, so nothing lands in private memory through a dynamic index.  Compiled with g++ under
// BH_HOSTSIM by tests/hostsim/posterior_sim.cpp (test infrastructure only).  Keys and binning: stats_core.h.
#pragma once
#include <stdint.h>
#include "bh_common.h"
#include "stats_core.h"

// member functions (BH_HD is `static inline` in the host build)
#if defined(BH_HOSTSIM)
#define BH_POST_M inline
#else
#define BH_POST_M __host__ __device__ __forceinline__
#endif

namespace bh {

// Leading non-NaN values of a row (the layout stores them first): 2 * nuclei, 0 for an all-NaN row.
template <typename T>
BH_HD int post_row_count(const T *row, int width)
{
    int c = 0;
    while (c < width && row[c] == row[c]) c++;
    return c;
}

// The merge of an ascending depth grid with a row's interfaces.  n nuclei, vs at row[k], z_vnoi at
// row[zoff + k]; k is the layer the walk stands in, D the depth of interface k (valid for k < n - 1).
template <typename T>
struct PostWalk {
    const T *row;
    int n, zoff, k;
    double D, disc;

    BH_POST_M void init(const T *r, int count)
    {
        row = r;
        n = count / 2;
        zoff = count - n;               // model[-n:] of split_modelparams
        k = 0;
        disc = 0.0;
        D = 0.0;
        if (n > 1) {
            disc = ((double)row[zoff] + (double)row[zoff + 1]) / 2.0;
            D = disc - 0.0;             // cumsum starts with h[0] = z_disc[0] - 0
        }
    }
    // cross interface k: D_{k+1} = D_k + (z_disc[k+1] - z_disc[k]), numpy's cumsum order
    BH_POST_M void cross()
    {
        k++;
        if (k < n - 1) {
            double nd = ((double)row[zoff + k] + (double)row[zoff + k + 1]) / 2.0;
            D = D + (nd - disc);
            disc = nd;
        }
    }
    // Vs at depth x; calls must come with non-decreasing x
    BH_POST_M T at(double x)
    {
        while (k < n - 1 && D <= x) cross();
        return row[k];
    }
    BH_POST_M bool has_interface() const { return k < n - 1; }
};

}  // namespace bh
