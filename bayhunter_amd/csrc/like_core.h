// like_core.h -- the pieces of like_kernel (like_kernel.hip) that know how many samples a row has: the residual
// that is staged into LDS, a lane's share of the closed forms, and the figures that follow from (sum d^2, q).
// (like_kernel itself, the form for calls without gaps, keeps its own text: its code object is to stay what it was.)
// like_kernel.hip compiles them for gfx950; tests/hostsim/like_gaps_sim.cpp compiles the very same functions with
// g++ (BH_HOSTSIM) and replays a workgroup's staging and wave sums on the host.
//
// DATA GAPS.  An observation set (a station) may lack samples of a target.  Such a target is valued as the
// reference's Valuation (src/Targets.py:99-183) values it when those lines have been deleted from the data file:
// the residual vector is the n' kept samples in order, compacted, and every closed form runs on n' instead of n.
// Two device tables describe the kept samples (LikeGaps; like_gap_tables builds them on the host):
//   cols[nsets][set_stride]  in the target's own columns off .. off + n' - 1 of a set's row: the kept samples of
//                            that target, ascending, as indices 0 .. n - 1 into the target (the rest is not read)
//   cnt[nsets][ntargets]     n'
// Lane i of a wave takes elements i, i + 64, ... of the COMPACTED vector -- the order of every sum is that of an
// unmasked call on a target table, modelled rows and yobs that hold the kept columns only, and so are the bits.
#pragma once
#include "bh_common.h"

namespace bh {

struct LikeGaps {
    const int *cols;   // [nsets][set_stride]
    const int *cnt;    // [nsets][ntargets]
};

// element i of a row's residual vector; ymod, yobs (and cols) point at the target's first column
template <bool MASKED>
BH_HD double like_residual(const double *ymod, const double *yobs, const int *cols, int i)
{
    const int c = MASKED ? cols[i] : i;
    return ymod[c] - yobs[c];
}

// A lane's share of sum d^2 and of the quadratic form q over the n staged residuals d.
BH_HD void like_nocorr_lane(const double *d, int n, int lane, double &s2, double &q)
{
    for (int i = lane; i < n; i += 64) s2 += d[i] * d[i];
    q = s2;
}
// se: the scaled errors in the target's own columns (a kept sample's lies at its column, not at its rank)
template <bool MASKED>
BH_HD void like_scaled_lane(const double *d, int n, int lane, const double *se, const int *cols, double &s2, double &q)
{
    for (int i = lane; i < n; i += 64) {
        double dd = d[i] * d[i];
        s2 += dd;
        q += dd / se[MASKED ? cols[i] : i];
    }
}
// exponential law: R^-1 tridiagonal, src/Targets.py:130-137.  Neighbours in d are neighbours: the reference's
// correlation law goes by index, so a shortened file correlates the samples on both sides of a gap.
BH_HD void like_exp_lane(const double *d, int n, int lane, double r, double &s2, double &q)
{
    for (int i = lane; i < n; i += 64) {
        double dd = d[i] * d[i];
        s2 += dd;
        double diag = (i == 0 || i == n - 1) ? 1.0 : 1.0 + r * r;
        q += diag * dd;
        if (i + 1 < n) q -= 2.0 * r * d[i] * d[i + 1];
    }
}

// A target's part of logL and its rms from (sum d^2, q) over n samples, src/Targets.py:102,113-146,341-344.
// extra: logdet_extra, or the set's log(prod(scaled_err)); the exponential law does not read it.
BH_HD void like_target_part(int cov, int n, double s2, double q, double corr, double sigma, double extra, double &logl,
                            double &rms)
{
    double madist, logdet = (2.0 * n) * log(sigma);
    if (cov == 2) {
        madist = q / (sigma * sigma * (1.0 - corr * corr));
        logdet += (n - 1) * log(1.0 - corr * corr);
    } else {
        madist = q / (sigma * sigma);
        logdet += extra;
    }
    const double logl_part = -0.5 * (n * log(2.0 * 3.141592653589793) + logdet);
    logl = logl_part - madist / 2.0;
    rms = sqrt(s2 / n);
}

// The two tables of LikeGaps from present[nsets][set_stride] (bytes, != 0: the set has this sample; only the
// targets' columns are read).  TG: bh_like_target or LikeTargetDev.  Returns 0, or -- with the first offender in
// *bad_set, *bad_target, tables then unfinished -- 1: a dense-Gaussian (cov 3) target with a gap (its R^-1 belongs
// to one n and to contiguous indices), 2: a target without a kept sample.  *any_gap: some set lacks some sample.
template <class TG>
inline int like_gap_tables(int nsets, int set_stride, int ntargets, const TG *tg, const unsigned char *present,
                           int *cols, int *cnt, bool *any_gap, int *bad_set, int *bad_target)
{
    *any_gap = false;
    for (long k = 0; k < (long)nsets * set_stride; k++) cols[k] = 0;
    for (int s = 0; s < nsets; s++)
        for (int t = 0; t < ntargets; t++) {
            const unsigned char *p = present + (long)s * set_stride + tg[t].off;
            int *c = cols + (long)s * set_stride + tg[t].off;
            int kept = 0;
            for (int i = 0; i < tg[t].n; i++)
                if (p[i]) c[kept++] = i;
            cnt[(long)s * ntargets + t] = kept;
            *bad_set = s; *bad_target = t;
            if (kept < tg[t].n && tg[t].cov == 3) return 1;
            if (kept == 0) return 2;
            if (kept < tg[t].n) *any_gap = true;
        }
    return 0;
}

}  // namespace bh
