// like_capi.hip -- the likelihood entry points of the C ABI (include/bayhunter_amd.h).  Host code only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "host_common.h"
#include "kernels.h"
#include "like_core.h"

using bh::fail_arg_;

extern "C" {

size_t bh_likelihood_workspace_bytes(int B, int ntargets, const bh_like_target *targets)
{
    if (!targets || B <= 0) return 0;
    int groups = 0;                         // [ntargets][B][groups][2]: kernels.h, LikeArgs::gq
    for (int t = 0; t < ntargets; t++)
        if (targets[t].cov == BH_COV_GAUSS && targets[t].n > 0) groups = std::max(groups, bh::gq_groups_of(targets[t].n));
    return (size_t)ntargets * (size_t)B * 2 * (size_t)groups * sizeof(double);
}

int bh_likelihood_batch(int B, int ntargets, const bh_like_target *targets, const double *out,
                        int out_stride, const int *err, int nflags, const double *yobs,
                        const double *noise, const double *aux, double *logL, double *misfits,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    return bh_likelihood_stage(BH_LIKE_STAGE_GAUSS | BH_LIKE_STAGE_REST, B, ntargets, targets, out, out_stride, err, nflags,
                               yobs, noise, aux, logL, misfits, workspace, workspace_bytes, stream);
}

int bh_likelihood_stage(int stages, int B, int ntargets, const bh_like_target *targets, const double *out,
                        int out_stride, const int *err, int nflags, const double *yobs,
                        const double *noise, const double *aux, double *logL, double *misfits,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    return bh_likelihood_sets(stages, B, ntargets, targets, out, out_stride, err, nflags, 1, nullptr, yobs, out_stride,
                              nullptr, nullptr, noise, aux, logL, misfits, workspace, workspace_bytes, stream);
}

int bh_likelihood_sets(int stages, int B, int ntargets, const bh_like_target *targets, const double *out,
                       int out_stride, const int *err, int nflags, int nsets, const int *obs_id, const double *yobs,
                       int set_stride, const double *set_scale, const double *set_logdet, const double *noise,
                       const double *aux, double *logL, double *misfits, void *workspace, size_t workspace_bytes,
                       void *stream)
{
    return bh::likelihood_sets_(stages, B, ntargets, targets, out, out_stride, err, nflags, nsets, obs_id, yobs, set_stride,
                                set_scale, set_logdet, noise, aux, logL, misfits, workspace, workspace_bytes, nullptr,
                                nullptr, 0, nullptr, nullptr, stream);
}

size_t bh_likelihood_gaps_workspace_bytes(int nsets, int set_stride, int ntargets)
{
    if (nsets < 1 || set_stride < 1 || ntargets < 1) return 0;
    return ((size_t)nsets * (size_t)set_stride + (size_t)nsets * (size_t)ntargets) * sizeof(int);
}

int bh_likelihood_sets_gaps(int stages, int B, int ntargets, const bh_like_target *targets, const double *out,
                            int out_stride, const int *err, int nflags, int nsets, const int *obs_id, const double *yobs,
                            int set_stride, const double *set_scale, const double *set_logdet, const double *noise,
                            const double *aux, double *logL, double *misfits, void *workspace, size_t workspace_bytes,
                            const unsigned char *set_present, void *gaps_workspace, size_t gaps_workspace_bytes,
                            void *stream)
{
    return bh::likelihood_sets_(stages, B, ntargets, targets, out, out_stride, err, nflags, nsets, obs_id, yobs, set_stride,
                                set_scale, set_logdet, noise, aux, logL, misfits, workspace, workspace_bytes, set_present,
                                gaps_workspace, gaps_workspace_bytes, nullptr, nullptr, stream);
}

}  // extern "C"

// The kept-sample tables of like_core.h from set_present[nsets][set_stride], cols then cnt in one vector (the layout
// of bh_likelihood_gaps_workspace_bytes), after the refusals: a dense-Gaussian target with a gap, a target without
// a kept sample.  The targets have been checked against set_stride.  evalplan.hip: bh_eval_set_gaps.
int bh::like_gaps_derive(const char *who, int nsets, int set_stride, int ntargets, const bh_like_target *targets,
                         const unsigned char *set_present, std::vector<int> &tables, bool *any_gap)
{
    tables.assign((size_t)nsets * set_stride + (size_t)nsets * ntargets, 0);
    int s = 0, t = 0;
    const int rc = like_gap_tables(nsets, set_stride, ntargets, targets, set_present, tables.data(),
                                   tables.data() + (size_t)nsets * set_stride, any_gap, &s, &t);
    if (rc == 1)
        return fail_arg_((std::string(who) + ": set " + std::to_string(s) + ", target " + std::to_string(t) +
                          " is BH_COV_GAUSS and has a gap (its dense R^-1 belongs to one n and to contiguous samples)").c_str());
    if (rc == 2)
        return fail_arg_((std::string(who) + ": set " + std::to_string(s) + ", target " + std::to_string(t) +
                          " has no sample left (set_present is 0 in all its columns)").c_str());
    return BH_OK;
}

// bh_likelihood_sets and bh_likelihood_sets_gaps.  The gaps come as set_present (HOST) with a device workspace for
// the tables derived from it, or as tables that are on the device already (gap_cols, gap_cnt: an evaluation plan's).
int bh::likelihood_sets_(int stages, int B, int ntargets, const bh_like_target *targets, const double *out, int out_stride,
                         const int *err, int nflags, int nsets, const int *obs_id, const double *yobs, int set_stride,
                         const double *set_scale, const double *set_logdet, const double *noise, const double *aux,
                         double *logL, double *misfits, void *workspace, size_t workspace_bytes,
                         const unsigned char *set_present, void *gaps_workspace, size_t gaps_workspace_bytes,
                         const int *gap_cols, const int *gap_cnt, void *stream)
{
    if (stages < 1 || stages > 3) return fail_arg_("bh_likelihood_stage: stages is BH_LIKE_STAGE_GAUSS | BH_LIKE_STAGE_REST");
    if (B < 0 || ntargets < 1 || ntargets > BH_MAX_TARGETS) return fail_arg_("B/ntargets out of range");
    if (nsets < 1) return fail_arg_("bh_likelihood_sets: nsets < 1");
    if (B == 0) return BH_OK;
    if (!targets || !out || !yobs || !noise || !logL || !misfits) return fail_arg_("NULL pointer");
    if (nflags < 0 || (nflags > 0 && !err)) return fail_arg_("err is NULL but nflags > 0");
    if (nsets > 1 && !obs_id) return fail_arg_("bh_likelihood_sets: obs_id is NULL but nsets > 1");
    if (!set_scale != !set_logdet) return fail_arg_("bh_likelihood_sets: set_scale and set_logdet come together");
    bh::LikeArgs A;
    std::memset(&A, 0, sizeof(A));
    int nmax = 1;
    for (int t = 0; t < ntargets; t++) {
        const bh_like_target &s = targets[t];
        if (s.n < 1 || s.n > bh::LIKE_NMAX) return fail_arg_("target size out of range (1..1024)");
        if (s.off < 0 || s.off + s.n > out_stride) return fail_arg_("target does not fit the output row");
        if (s.off + s.n > set_stride) return fail_arg_("bh_likelihood_sets: target does not fit a set's row (set_stride)");
        if (s.cov < 0 || s.cov > 3) return fail_arg_("unknown covariance model");
        if (s.cov == BH_COV_NOCORR_SCALED && nsets > 1 && !set_scale)
            return fail_arg_("bh_likelihood_sets: a BH_COV_NOCORR_SCALED target needs set_scale and set_logdet with nsets > 1");
        if (((s.cov == BH_COV_NOCORR_SCALED && !set_scale) || s.cov == BH_COV_GAUSS) && !aux) return fail_arg_("aux is NULL");
        A.tg[t] = bh::LikeTargetDev{s.n, s.off, s.cov, s.aux_off, s.logdet_extra};
        if (s.n > nmax) nmax = s.n;
    }
    bh::LikeGaps G{gap_cols, gap_cnt};
    bool masked = gap_cols && gap_cnt;
    std::vector<int> tables;
    if (set_present) {
        const size_t need = bh_likelihood_gaps_workspace_bytes(nsets, set_stride, ntargets);
        if (!gaps_workspace || gaps_workspace_bytes < need) {
            fail_arg_("bh_likelihood_sets_gaps: gaps_workspace is NULL or smaller than bh_likelihood_gaps_workspace_bytes()");
            return BH_ERR_WORKSPACE;
        }
        if (int rc = like_gaps_derive("bh_likelihood_sets_gaps", nsets, set_stride, ntargets, targets, set_present, tables, &masked))
            return rc;
        G.cols = (const int *)gaps_workspace;
        G.cnt = G.cols + (size_t)nsets * set_stride;
    }
    int rc = require_device();
    if (rc) return rc;
    A.B = B; A.ntargets = ntargets; A.out_stride = out_stride; A.nflags = nflags;
    A.out = out; A.err = err; A.yobs = yobs; A.noise = noise; A.aux = aux;
    A.nsets = nsets; A.set_stride = set_stride; A.obs_id = obs_id; A.set_scale = set_scale; A.set_logdet = set_logdet;
    A.logL = logL; A.misfits = misfits;
    size_t need = bh_likelihood_workspace_bytes(B, ntargets, targets);
    A.gq = (need > 0 && workspace && workspace_bytes >= need) ? (double *)workspace : nullptr;
    A.gq_groups = (int)(need / ((size_t)ntargets * (size_t)B * 2 * sizeof(double)));
    if (stages != 3 && !A.gq) return fail_arg_("bh_likelihood_stage: the stages can only be split with a workspace");
    masked = masked && (stages & BH_LIKE_STAGE_REST);        // (the dense products have no gaps)
    if (masked && set_present) {
        // in stream order behind whatever still reads the workspace; the host copy goes when this call returns
        BH_HIP(hipMemcpyAsync(gaps_workspace, tables.data(), tables.size() * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
        BH_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    BH_HIP(bh::launch_like(A, nmax, (hipStream_t)stream, stages, masked ? &G : nullptr));
    return BH_OK;
}
