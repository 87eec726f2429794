// evalplan.hip -- one call per batch of proposals: pinned host block -> HBM -> processing order ->
// dispersion / receiver-function / likelihood kernels -> 8*(ntargets+2) bytes per model back.
//
// The sampler's per-iteration hand-over (reference: SingleChain.iterate -> JointTarget.evaluate, one model
// per call, src/SingleChain.py:511-589, src/Targets.py:314-347).  The chain pool used to drive this from
// Python: a dozen torch calls per batch (copies, views, argsort, allocation, events), 0.19 s of host time
// for 150 iterations of 4 096 chains -- as long as the device needed for the arithmetic.  A plan owns
// everything a batch needs (device buffers, pinned staging, two streams, events, sort scratch), so a
// submission is: three async copies (or one), at most seven kernel launches, one async copy back, one
// event.  No allocation, no Python object, no torch in the loop.
// The forward stage of a submission is bh_forward_batch, which ForwardEngine.run (bayhunter_amd/engine.py) calls too.
#include <hip/hip_runtime.h>
#include <cstring>                     // (before rocprim: its texture iterator calls the host memset)
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>
#include "host_common.h"

namespace {

constexpr int kOrderMin = 1024;   // up to this every team is resident at once: order is irrelevant (layout.py: ORDER_MIN)

// numpy.interp(obsx, xp, f) for the n values f solved at xp (a target with more than 60 periods); an observed period on
// the last solved one takes f[n-1] (numpy/core/src/multiarray/compiled_base.c: arr_interp).  Exactly rounded
// subtractions and comparisons, no fused multiply-add (-ffp-contract=off): the bits of numpy.interp on the host.
__global__ void interp_kernel(int B, double *out, int stride, const double *xp, int n, int src_off, bh_eval_interp d)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * d.n_dst) return;
    const int b = (int)(idx / d.n_dst), i = (int)(idx - (long)b * d.n_dst);
    const double x = d.obsx[i];
    int j = 0;                                     // searchsorted(xp, x, 'right'): xp is sorted, n <= 60
    for (int k = 0; k < n; k++) j += !(x < xp[k]);
    j = min(max(j - 1, 0), n - 2);
    double *row = out + (long)b * stride;
    const double *f = row + src_off;
    const double f0 = f[j], f1 = f[j + 1];
    const double y = ((f1 - f0) / (xp[j + 1] - xp[j])) * (x - xp[j]) + f0;
    row[d.dst_off + i] = x == xp[n - 1] ? f[n - 1] : y;
}

// Without a dispersion target no kernel raises BH_MODEL_BAD_DEPTH: the flag of a model whose layer count is outside
// 1..L (its receiver-function row is NaN) is set here.  err has one column then.
__global__ void depth_flags_kernel(int n, const int *nlay, int L, int *err)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) err[i] = (nlay[i] < 1 || nlay[i] > L) ? BH_MODEL_BAD_DEPTH : 0;
}

__global__ void iota_kernel(int n, int *v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

}  // namespace

struct bh_eval_plan {
    int dev = 0, rows = 0, Lmax = 0, row = 0, nswd = 0, nrf = 0, T = 0, nflags = 0, use_mfma = 1;
    double tmax = 0.0;
    std::vector<bh_swd_target> swd;
    std::vector<bh_rf_params> rf;
    std::vector<bh_like_target> like;
    std::vector<bh_eval_interp> interp;   // obsx: device pointers into `obsx`
    // pinned host staging: [packed rows*4*Lmax | noise rows*2T] doubles, then [nlay rows | set rows | chain rows] ints
    // (set: the observation set of each row, filled by bh_eval_submit from chain[] once bh_eval_set_observations was called)
    char *hblock = nullptr;
    size_t off_noise = 0, off_nlay = 0, off_set = 0, off_chain = 0, hbytes = 0;
    double *hres = nullptr;       // [rows] logL, then [rows][T+1] misfits of the last submission
    // device
    char *dblock = nullptr;       // same layout as hblock up to the end of set
    double *periods = nullptr, *obsx = nullptr, *yobs = nullptr, *aux = nullptr, *out = nullptr, *dres = nullptr;
    int *err = nullptr, *keys = nullptr, *keys_out = nullptr, *iota = nullptr, *order = nullptr;
    void *sort_tmp = nullptr, *like_ws = nullptr, *swd_ws = nullptr;
    size_t sort_bytes = 0, like_bytes = 0, swd_bytes = 0;
    hipStream_t st = nullptr, side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, done = nullptr;
    int concurrency = 1;          // plans taking turns on the device (bh_eval_set_concurrency)
    bool gauss_on_side = false;   // every dense-Gaussian target is a receiver function's: its product runs behind
                                  // rf_kernel on the side stream, beside the dispersion searches (bh_eval_submit)
    // observation sets (bh_eval_set_observations): yobs holds nsets rows; set_of_chain maps chain[k] to its set
    int nsets = 1;
    double *set_scale = nullptr, *set_logdet = nullptr;
    std::vector<int> set_of_chain;
    double *rf_set_p = nullptr;   // [nrf][nsets] ray parameters per set (bh_eval_set_rf_slowness), or null: rf[i].p
    int *gaps = nullptr;          // [nsets][row] columns of the kept samples, then [nsets][T] their counts
                                  // (bh_eval_set_gaps; like_core.h), or null: no set has a gap
    bool gaps_set = false;        // bh_eval_set_gaps has been called (a table without a gap leaves `gaps` null)
    std::vector<bh_ell_target> ell;   // ellipticity targets (bh_eval_set_ellipticity): one ell_rows_kernel each, behind
                                      // the dispersion stage on `st`
    bool submitted = false;       // a batch has been submitted: the observations are fixed from then on
    int last_count = 0;           // models of the submission `done` belongs to (set once `done` is recorded)
    bool failed = false;          // the last submission returned an error: nothing to wait for, no results
    std::string failure;
};

static void plan_free(bh_eval_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->dev);
    if (p->st) (void)hipStreamSynchronize(p->st);
    if (p->side) (void)hipStreamSynchronize(p->side);
    void *dptr[] = {p->dblock, p->periods, p->obsx, p->yobs, p->aux, p->set_scale, p->set_logdet, p->rf_set_p, p->gaps, p->out, p->dres, p->err, p->keys,
                    p->keys_out, p->iota, p->order, p->sort_tmp, p->like_ws, p->swd_ws};
    for (void *d : dptr)
        if (d) (void)hipFree(d);
    if (p->hblock) (void)hipHostFree(p->hblock);
    if (p->hres) (void)hipHostFree(p->hres);
    if (p->fork) (void)hipEventDestroy(p->fork);
    if (p->join) (void)hipEventDestroy(p->join);
    if (p->done) (void)hipEventDestroy(p->done);
    // the library's own events on these streams (work-queue slot guards, swd_launch.hip) go before the streams do
    if (p->st) (void)bh_stream_retire(p->st);
    if (p->side) (void)bh_stream_retire(p->side);
    if (p->st) (void)hipStreamDestroy(p->st);
    if (p->side) (void)hipStreamDestroy(p->side);
    delete p;
}

template <class T>
static int upload(T **d, const T *h, size_t n)
{
    BH_HIP(hipMalloc((void **)d, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) BH_HIP(hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return BH_OK;
}

// an interpolation names a dispersion target of at least two periods and columns inside the output row
static int check_interp(int nswd, const bh_swd_target *swd, int out_stride, int ninterp, const bh_eval_interp *interp)
{
    for (int i = 0; i < ninterp; i++) {
        const bh_eval_interp &s = interp[i];
        if (s.target < 0 || s.target >= nswd || swd[s.target].nper < 2 || !s.obsx || s.n_dst < 1 || s.dst_off < 0 ||
            s.dst_off + s.n_dst > out_stride)
            return bh::fail_arg_("bad interpolation descriptor");
    }
    return BH_OK;
}

extern "C" {

int bh_eval_create(int max_models, int Lmax, int row, int nswd, const bh_swd_target *swd,
                   const double *periods, int nperiods, int nrf, const bh_rf_params *rf, int ntargets,
                   const bh_like_target *like, int nflags, const double *yobs, const double *aux,
                   size_t naux, int ninterp, const bh_eval_interp *interp, int use_mfma,
                   bh_eval_plan **plan)
{
    if (!plan) return bh::fail_arg_("plan is NULL");
    *plan = nullptr;
    if (max_models < 1 || Lmax < 1 || Lmax > BH_MAX_LAYERS || row < 1) return bh::fail_arg_("max_models/Lmax/row out of range");
    if (nswd < 0 || nswd > BH_MAX_TARGETS || nrf < 0 || nswd + nrf < 1) return bh::fail_arg_("no forward targets");
    if (ntargets < 1 || ntargets > BH_MAX_TARGETS || !like || !yobs) return bh::fail_arg_("likelihood targets missing");
    if ((nswd && (!swd || !periods)) || (nrf && !rf) || (ninterp && !interp)) return bh::fail_arg_("NULL pointer");
    if (nflags != (nswd > 0 ? nswd : 1)) return bh::fail_arg_("nflags must be the number of dispersion targets (1 without any)");
    if (int rc = check_interp(nswd, swd, row, ninterp, interp)) return rc;
    if (int rc = bh::require_device()) return rc;
    bh_eval_plan *p = new (std::nothrow) bh_eval_plan;
    if (!p) return bh::fail_arg_("out of memory");
    int rc = BH_OK;
    auto bail = [&](int code) { plan_free(p); return code; };
    if (hipGetDevice(&p->dev) != hipSuccess) return bail(bh::fail_arg_("hipGetDevice failed"));
    p->rows = max_models; p->Lmax = Lmax; p->row = row; p->nswd = nswd; p->nrf = nrf; p->T = ntargets;
    p->nflags = nflags; p->use_mfma = use_mfma;
    p->swd.assign(swd, swd + nswd);
    p->rf.assign(rf, rf + nrf);
    p->like.assign(like, like + ntargets);
    for (int t = 0; t < nswd; t++) {
        if (swd[t].per_off < 0 || swd[t].nper < 0 || swd[t].per_off + swd[t].nper > nperiods)
            return bail(bh::fail_arg_("a target's periods lie outside the period array"));
        for (int k = 0; k < swd[t].nper; k++) p->tmax = std::max(p->tmax, periods[swd[t].per_off + k]);
    }
    const size_t R = (size_t)max_models;
    p->off_noise = R * 4 * Lmax * sizeof(double);
    p->off_nlay = p->off_noise + R * 2 * ntargets * sizeof(double);
    p->off_set = p->off_nlay + R * sizeof(int);
    p->off_chain = p->off_set + R * sizeof(int);
    p->hbytes = p->off_chain + R * sizeof(int);
    if (hipHostMalloc((void **)&p->hblock, p->hbytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&p->hres, R * (ntargets + 2) * sizeof(double), hipHostMallocDefault) != hipSuccess)
        return bail(bh::fail_hip_((int)hipErrorOutOfMemory, "hipHostMalloc(staging)"));
    std::memset(p->hblock, 0, p->hbytes);
    if (hipMalloc((void **)&p->dblock, p->off_chain) != hipSuccess ||
        hipMalloc((void **)&p->out, R * row * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&p->err, R * nflags * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&p->dres, R * (ntargets + 2) * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&p->keys, R * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&p->keys_out, R * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&p->iota, R * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&p->order, R * sizeof(int)) != hipSuccess)
        return bail(bh::fail_hip_((int)hipErrorOutOfMemory, "hipMalloc(plan buffers)"));
    if ((rc = upload(&p->periods, periods, (size_t)(nswd ? nperiods : 0)))) return bail(rc);
    if ((rc = upload(&p->yobs, yobs, (size_t)row))) return bail(rc);
    if ((rc = upload(&p->aux, aux, aux ? naux : 0))) return bail(rc);
    std::vector<double> obsx;                        // every target's observed periods, uploaded once
    for (int i = 0; i < ninterp; i++) obsx.insert(obsx.end(), interp[i].obsx, interp[i].obsx + interp[i].n_dst);
    if ((rc = upload(&p->obsx, obsx.data(), obsx.size()))) return bail(rc);
    p->interp.assign(interp, interp + ninterp);
    for (size_t i = 0, off = 0; i < p->interp.size(); off += p->interp[i++].n_dst) p->interp[i].obsx = p->obsx + off;
    p->like_bytes = use_mfma ? bh_likelihood_workspace_bytes(max_models, ntargets, like) : 0;
    p->swd_bytes = nswd ? bh_swd_workspace_bytes(max_models, nswd, swd) : 0;
    if ((p->like_bytes && hipMalloc(&p->like_ws, p->like_bytes) != hipSuccess) ||
        (p->swd_bytes && hipMalloc(&p->swd_ws, p->swd_bytes) != hipSuccess))
        return bail(bh::fail_hip_((int)hipErrorOutOfMemory, "hipMalloc(workspaces)"));
    // The receiver-function kernel only back-fills the draining tail of the dispersion kernel when the two
    // streams differ in priority: two plain streams behaved like one (68.1 vs 66.0 ms per 524 288-model step,
    // tools/prio_exp.py), apparently sharing a hardware queue.
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (hipStreamCreateWithPriority(&p->st, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipEventCreateWithFlags(&p->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->done, hipEventDisableTiming) != hipSuccess)
        return bail(bh::fail_hip_((int)hipErrorUnknown, "stream / event creation"));
    if (p->like_bytes && nswd > 0 && nrf > 0) {
        bool all_rf = true, any = false;
        for (int t = 0; t < ntargets; t++) {
            if (like[t].cov != BH_COV_GAUSS) continue;
            any = true;
            bool in_rf = false;
            for (int i = 0; i < nrf; i++)
                in_rf = in_rf || (like[t].off >= rf[i].out_off && like[t].off + like[t].n <= rf[i].out_off + rf[i].nout);
            all_rf = all_rf && in_rf;
        }
        p->gauss_on_side = any && all_rf;
    }
    hipLaunchKernelGGL(iota_kernel, dim3((max_models + 255) / 256), dim3(256), 0, p->st, max_models, p->iota);
    if (max_models > kOrderMin && nswd) {
        if (rocprim::radix_sort_pairs(nullptr, p->sort_bytes, p->keys, p->keys_out, p->iota, p->order,
                                      (size_t)max_models, 0, 32, p->st) != hipSuccess ||
            hipMalloc(&p->sort_tmp, std::max<size_t>(p->sort_bytes, 16)) != hipSuccess)
            return bail(bh::fail_hip_((int)hipErrorOutOfMemory, "radix sort scratch"));
    }
    if (hipStreamSynchronize(p->st) != hipSuccess) return bail(bh::fail_hip_((int)hipErrorUnknown, "plan set-up"));
    *plan = p;
    return BH_OK;
}

void bh_eval_destroy(bh_eval_plan *plan) { plan_free(plan); }

int bh_eval_buffers(bh_eval_plan *p, double **packed, int **nlay, double **noise, int **chain,
                    double **results)
{
    if (!p) return bh::fail_arg_("plan is NULL");
    if (packed) *packed = (double *)p->hblock;
    if (noise) *noise = (double *)(p->hblock + p->off_noise);
    if (nlay) *nlay = (int *)(p->hblock + p->off_nlay);
    if (chain) *chain = (int *)(p->hblock + p->off_chain);
    if (results) *results = p->hres;
    return BH_OK;
}

}  // extern "C"

// bh_forward_batch, and the plan's forward stage with per-set ray parameters: rf_set_p [nrf][nsets] and set_id [B]
// (DEVICE; bh_eval_set_rf_slowness) send every receiver-function target through bh_rf_batch_sets.
static int forward_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp,
                         const double *vs, const double *rho, int nswd, const bh_swd_target *swd, const double *periods,
                         int ninterp, const bh_eval_interp *interp, int nrf, const bh_rf_params *rf, const int *order,
                         double mean_layers, int concurrent_calls, double *out, int out_stride, int *err, void *workspace,
                         size_t workspace_bytes, void *stream, void *rf_stream, int nsets, const double *rf_set_p,
                         const int *set_id)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return bh::fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return bh::fail_arg_("model_stride < Lmax");
    if (nswd < 0 || nswd > BH_MAX_TARGETS || nrf < 0 || nswd + nrf < 1) return bh::fail_arg_("no forward targets");
    if (B == 0) return BH_OK;
    if (!nlay || !h || !vp || !vs || !rho || !out || !err || (nswd && (!swd || !periods)) || (nrf && !rf) ||
        (ninterp && !interp))
        return bh::fail_arg_("NULL pointer");
    // the dispersion targets are checked by bh_swd_batch_ordered, before its launch: the first one
    int rc = check_interp(nswd, swd, out_stride, ninterp, interp);
    for (int i = 0; i < nrf && !rc; i++) rc = bh::check_rf_params(rf + i, Lmax, out_stride, false);
    if (rc) return rc;
    if (nswd) {
        if ((rc = bh_swd_hint(mean_layers, concurrent_calls))) return rc;
        if ((rc = bh_swd_batch_ordered(B, Lmax, model_stride, nlay, h, vp, vs, rho, nswd, swd, periods, out, out_stride,
                                       err, order, workspace, workspace_bytes, stream)))
            return rc;
        for (int i = 0; i < ninterp; i++) {
            const bh_swd_target &t = swd[interp[i].target];
            const long n = (long)B * interp[i].n_dst;
            hipLaunchKernelGGL(interp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B,
                               out, out_stride, periods + t.per_off, t.nper, t.out_off, interp[i]);
            BH_HIP(hipGetLastError());
        }
    } else {
        hipLaunchKernelGGL(depth_flags_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B,
                           nlay, Lmax, err);
        BH_HIP(hipGetLastError());
    }
    for (int i = 0; i < nrf; i++) {
        rc = rf_set_p ? bh_rf_batch_sets(B, Lmax, model_stride, nlay, h, vp, vs, rho, nullptr, nullptr, rf + i, nsets,
                                         rf_set_p + (size_t)i * nsets, set_id, out, out_stride, nullptr, 0, rf_stream)
                      : bh_rf_batch(B, Lmax, model_stride, nlay, h, vp, vs, rho, nullptr, nullptr, rf + i, out, out_stride,
                                    nullptr, 0, rf_stream);
        if (rc) return rc;
    }
    return BH_OK;
}

extern "C" {

int bh_forward_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp,
                     const double *vs, const double *rho, int nswd, const bh_swd_target *swd, const double *periods,
                     int ninterp, const bh_eval_interp *interp, int nrf, const bh_rf_params *rf, const int *order,
                     double mean_layers, int concurrent_calls, double *out, int out_stride, int *err, void *workspace,
                     size_t workspace_bytes, void *stream, void *rf_stream)
{
    return forward_batch(B, Lmax, model_stride, nlay, h, vp, vs, rho, nswd, swd, periods, ninterp, interp, nrf, rf, order,
                         mean_layers, concurrent_calls, out, out_stride, err, workspace, workspace_bytes, stream, rf_stream,
                         0, nullptr, nullptr);
}

int bh_forward_batch_sets(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp,
                          const double *vs, const double *rho, int nswd, const bh_swd_target *swd, const double *periods,
                          int ninterp, const bh_eval_interp *interp, int nrf, const bh_rf_params *rf, const int *order,
                          double mean_layers, int concurrent_calls, double *out, int out_stride, int *err, void *workspace,
                          size_t workspace_bytes, void *stream, void *rf_stream, int nsets, const double *rf_set_p,
                          const int *set_id)
{
    if (rf_set_p) {                        // (what bh_rf_batch_sets would refuse only after the dispersion launch)
        if (nrf < 1) return bh::fail_arg_("bh_forward_batch_sets: ray parameters without a receiver-function target");
        if (nsets < 1) return bh::fail_arg_("bh_forward_batch_sets: nsets < 1");
        if (!set_id && nsets > 1) return bh::fail_arg_("bh_forward_batch_sets: set_id is NULL with more than one set");
    }
    return forward_batch(B, Lmax, model_stride, nlay, h, vp, vs, rho, nswd, swd, periods, ninterp, interp, nrf, rf, order,
                         mean_layers, concurrent_calls, out, out_stride, err, workspace, workspace_bytes, stream, rf_stream,
                         rf_set_p ? nsets : 0, rf_set_p, rf_set_p ? set_id : nullptr);
}

}  // extern "C"

// the launches of one submission; `forked` tells the caller whether the side stream was made to wait
static int submit_batch(bh_eval_plan *p, int count, bool *forked)
{
    BH_HIP(hipSetDevice(p->dev));
    const int L = p->Lmax, T = p->T;
    const int *hnlay = (const int *)(p->hblock + p->off_nlay);
    int depth = 1;
    long layers = 0;
    for (int i = 0; i < count; i++) { depth = std::max(depth, hnlay[i]); layers += hnlay[i] > 0 ? hnlay[i] : 0; }
    // the kernels size their LDS images by the deepest model of the batch (even, so that rows can be
    // fetched two layers at a time), not by the allocated row length
    const int Leff = std::min(L, depth + (depth & 1));
    // small pools: the whole block in one copy; large ones: only the used part of each section
    const bool sets = !p->set_of_chain.empty();
    if (sets) {                            // one int per row: the set of the chain the proposal belongs to
        const int *chain = (const int *)(p->hblock + p->off_chain);
        int *set = (int *)(p->hblock + p->off_set);
        const int nchains = (int)p->set_of_chain.size();
        for (int k = 0; k < count; k++) {
            if (chain[k] < 0 || chain[k] >= nchains) return bh::fail_arg_("bh_eval_submit: chain[] names a chain outside bh_eval_set_observations' set_of_chain");
            set[k] = p->set_of_chain[chain[k]];
        }
    }
    if (p->rows <= 16384) {
        BH_HIP(hipMemcpyAsync(p->dblock, p->hblock, (sets ? p->off_set : p->off_nlay) + (size_t)count * sizeof(int),
                              hipMemcpyHostToDevice, p->st));
    } else {
        if (sets)
            BH_HIP(hipMemcpyAsync(p->dblock + p->off_set, p->hblock + p->off_set, (size_t)count * sizeof(int),
                                  hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemcpyAsync(p->dblock, p->hblock, (size_t)count * 4 * L * sizeof(double), hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemcpyAsync(p->dblock + p->off_noise, p->hblock + p->off_noise, (size_t)count * 2 * T * sizeof(double),
                              hipMemcpyHostToDevice, p->st));
        BH_HIP(hipMemcpyAsync(p->dblock + p->off_nlay, p->hblock + p->off_nlay, (size_t)count * sizeof(int),
                              hipMemcpyHostToDevice, p->st));
    }
    const double *dm = (const double *)p->dblock;
    const double *dnoise = (const double *)(p->dblock + p->off_noise);
    const int *dnlay = (const int *)(p->dblock + p->off_nlay);
    const int *dset = sets ? (const int *)(p->dblock + p->off_set) : nullptr;
    const double *h = dm, *vp = dm + L, *vs = dm + 2 * L, *rho = dm + 3 * L;
    int rc;
    const bool overlap = p->nswd > 0 && p->nrf > 0;
    if (overlap) {
        BH_HIP(hipEventRecord(p->fork, p->st));
        BH_HIP(hipStreamWaitEvent(p->side, p->fork, 0));
        *forked = true;
    }
    const int *order = nullptr;
    if (p->nswd && count > kOrderMin) {   // deepest first, longest searches first, alike neighbours (engine.reorder)
        if ((rc = bh_swd_order_keys(count, L, 4 * L, dnlay, h, vs, p->tmax, 1, p->keys, p->st))) return rc;
        size_t bytes = p->sort_bytes;
        BH_HIP(rocprim::radix_sort_pairs(p->sort_tmp, bytes, p->keys, p->keys_out, p->iota, p->order,
                                         (size_t)count, 0, 32, p->st));
        order = p->order;
    }
    // the batch is ragged: the planner prices it by its mean depth, not by its deepest model (swd_launch.hip: plan_forms)
    hipStream_t rst = overlap ? p->side : p->st;
    if ((rc = forward_batch(count, Leff, 4 * L, dnlay, h, vp, vs, rho, p->nswd, p->swd.data(), p->periods,
                            (int)p->interp.size(), p->interp.data(), p->nrf, p->rf.data(), order,
                            (double)layers / (double)count, p->concurrency, p->out, p->row, p->err, p->swd_ws,
                            p->swd_bytes, p->st, rst, p->nsets, p->rf_set_p, dset)))
        return rc;
    // The ellipticities: behind the dispersion searches (and the interpolations) on their stream, in front of the
    // join, so that the receiver functions on the side stream run beside them.  A model without a value gets
    // BH_ELL_NO_VALUE in its source target's flag, which the likelihood behind the join reads.
    for (const bh_ell_target &e : p->ell) {
        const bh_swd_target &src = p->swd[e.src];
        if ((rc = bh_ell_batch_rows(count, Leff, 4 * L, dnlay, h, vp, vs, rho, e.nper, p->periods + src.per_off, src.iflsph,
                                    p->out + src.out_off, p->row, p->err + e.src, p->nflags, e.absolute, p->out + e.out_off,
                                    p->row, order, 1, p->st)))
            return rc;
    }
    double *logL = p->dres, *mis = p->dres + count;
    // The dense Gaussian product of a receiver-function target needs that target's columns only: it follows
    // rf_kernel on the side stream, beside this batch's dispersion searches.  Behind the join it was on the critical
    // path of every batch -- and, a short kernel that asks for four SIMDs' worth of registers at once, it waited a
    // third of a millisecond for the OTHER chain group's teams to drain (rocprofv3 of a 4 096-chain pool: 0.31 ms per
    // call where it takes 0.04 ms alone, 22 % of the kernel time).
    const bool staged = overlap && p->gauss_on_side;
    const int *gcols = p->gaps, *gcnt = p->gaps ? p->gaps + (size_t)p->nsets * p->row : nullptr;
    if (staged && (rc = bh::likelihood_sets_(BH_LIKE_STAGE_GAUSS, count, T, p->like.data(), p->out, p->row, p->err, p->nflags,
                                             p->nsets, dset, p->yobs, p->row, p->set_scale, p->set_logdet, dnoise, p->aux,
                                             logL, mis, p->like_ws, p->like_bytes, nullptr, nullptr, 0, gcols, gcnt, rst)))
        return rc;
    if (overlap) {
        BH_HIP(hipEventRecord(p->join, p->side));
        BH_HIP(hipStreamWaitEvent(p->st, p->join, 0));
        *forked = false;                  // joined
    }
    if ((rc = bh::likelihood_sets_(staged ? BH_LIKE_STAGE_REST : (BH_LIKE_STAGE_GAUSS | BH_LIKE_STAGE_REST), count, T,
                                   p->like.data(), p->out, p->row, p->err, p->nflags, p->nsets, dset, p->yobs, p->row,
                                   p->set_scale, p->set_logdet, dnoise, p->aux, logL, mis, p->like_ws, p->like_bytes,
                                   nullptr, nullptr, 0, gcols, gcnt, p->st)))
        return rc;
    // results: [count] logL then [count][T+1] misfits, contiguous on both sides
    BH_HIP(hipMemcpyAsync(p->hres, p->dres, (size_t)count * (T + 2) * sizeof(double), hipMemcpyDeviceToHost, p->st));
    BH_HIP(hipEventRecord(p->done, p->st));
    return BH_OK;
}

extern "C" {

int bh_eval_submit(bh_eval_plan *p, int count)
{
    if (!p) return bh::fail_arg_("plan is NULL");
    if (count < 0 || count > p->rows) return bh::fail_arg_("count out of range");
    p->failed = false;
    p->last_count = 0;
    p->submitted = true;
    if (count == 0) return BH_OK;
    bool forked = false;
    const int rc = submit_batch(p, count, &forked);
    if (rc != BH_OK) {
        // Nothing of this submission may be mistaken for a result: bh_eval_wait reports the failure instead of
        // finding a stale (or never recorded, hence "complete") event.  What was queued is drained: the side stream
        // may already be waiting on `fork`, so the main stream joins it before the plan is used or freed.
        p->failed = true;
        p->failure = bh_last_error();
        if (forked && hipEventRecord(p->join, p->side) == hipSuccess) (void)hipStreamWaitEvent(p->st, p->join, 0);
        bh::fail_arg_(p->failure.c_str());           // (the calls above may have replaced the message)
        return rc;
    }
    p->last_count = count;                            // only now: `done` has been recorded for this batch
    return BH_OK;
}

int bh_eval_set_observations(bh_eval_plan *p, int nsets, const double *yobs, const double *set_scale,
                             const double *set_logdet, const int *set_of_chain, int nchains)
{
    if (nsets < 1) return bh::fail_arg_("bh_eval_set_observations: nsets < 1");
    if (!yobs || !set_of_chain) return bh::fail_arg_("bh_eval_set_observations: NULL pointer (yobs / set_of_chain)");
    if (nchains < 1) return bh::fail_arg_("bh_eval_set_observations: nchains < 1");
    if (!set_scale != !set_logdet) return bh::fail_arg_("bh_eval_set_observations: set_scale and set_logdet come together");
    for (int c = 0; c < nchains; c++)
        if (set_of_chain[c] < 0 || set_of_chain[c] >= nsets)
            return bh::fail_arg_(("bh_eval_set_observations: set_of_chain[" + std::to_string(c) + "] = " +
                                  std::to_string(set_of_chain[c]) + " is outside 0 .. nsets-1").c_str());
    if (!p) return bh::fail_arg_("plan is NULL");
    if (p->submitted) return bh::fail_arg_("bh_eval_set_observations: called after bh_eval_submit");
    if (!p->set_of_chain.empty()) return bh::fail_arg_("bh_eval_set_observations: the plan has its observation sets already");
    for (const bh_like_target &t : p->like)
        if (t.cov == BH_COV_NOCORR_SCALED && !set_scale)
            return bh::fail_arg_("bh_eval_set_observations: a BH_COV_NOCORR_SCALED target needs set_scale and set_logdet");
    BH_HIP(hipSetDevice(p->dev));
    double *dy = nullptr, *ds = nullptr, *dl = nullptr;
    int rc = upload(&dy, yobs, (size_t)nsets * p->row);
    if (!rc && set_scale) rc = upload(&ds, set_scale, (size_t)nsets * p->row);
    if (!rc && set_scale) rc = upload(&dl, set_logdet, (size_t)nsets * p->T);
    if (rc) {
        for (void *d : {(void *)dy, (void *)ds, (void *)dl})
            if (d) (void)hipFree(d);
        return rc;
    }
    (void)hipFree(p->yobs);
    p->yobs = dy; p->set_scale = ds; p->set_logdet = dl;
    p->nsets = nsets;
    p->set_of_chain.assign(set_of_chain, set_of_chain + nchains);
    return BH_OK;
}

int bh_eval_set_rf_slowness(bh_eval_plan *p, int nsets, const double *table)
{
    if (nsets < 1) return bh::fail_arg_("bh_eval_set_rf_slowness: nsets < 1");
    if (!table) return bh::fail_arg_("bh_eval_set_rf_slowness: NULL pointer (p)");
    if (!p) return bh::fail_arg_("plan is NULL");
    if (p->nrf < 1) return bh::fail_arg_("bh_eval_set_rf_slowness: the plan has no receiver-function target");
    if (p->submitted) return bh::fail_arg_("bh_eval_set_rf_slowness: called after bh_eval_submit");
    if (p->rf_set_p) return bh::fail_arg_("bh_eval_set_rf_slowness: the plan has its ray parameters already");
    if (p->set_of_chain.empty())
        return bh::fail_arg_("bh_eval_set_rf_slowness: call bh_eval_set_observations first (it tells the plan the set of every chain)");
    if (nsets != p->nsets)
        return bh::fail_arg_(("bh_eval_set_rf_slowness: nsets = " + std::to_string(nsets) + ", but bh_eval_set_observations gave the plan " +
                              std::to_string(p->nsets) + " sets").c_str());
    std::vector<double> byrf((size_t)p->nrf * nsets);          // [nrf][nsets]: one contiguous table per target
    for (int s = 0; s < nsets; s++)
        for (int i = 0; i < p->nrf; i++) {
            const double v = table[(size_t)s * p->nrf + i];
            if (!std::isfinite(v))
                return bh::fail_arg_(("bh_eval_set_rf_slowness: p[" + std::to_string(s) + "][" + std::to_string(i) +
                                      "] is not finite").c_str());
            byrf[(size_t)i * nsets + s] = v;
        }
    BH_HIP(hipSetDevice(p->dev));
    double *d = nullptr;
    if (int rc = upload(&d, byrf.data(), byrf.size())) {
        if (d) (void)hipFree(d);
        return rc;
    }
    p->rf_set_p = d;
    return BH_OK;
}

int bh_eval_set_gaps(bh_eval_plan *p, int nsets, const unsigned char *set_present)
{
    if (nsets < 1) return bh::fail_arg_("bh_eval_set_gaps: nsets < 1");
    if (!set_present) return bh::fail_arg_("bh_eval_set_gaps: NULL pointer (set_present)");
    if (!p) return bh::fail_arg_("plan is NULL");
    if (p->submitted) return bh::fail_arg_("bh_eval_set_gaps: called after bh_eval_submit");
    if (p->gaps_set) return bh::fail_arg_("bh_eval_set_gaps: the plan has its gaps already");
    if (p->set_of_chain.empty())
        return bh::fail_arg_("bh_eval_set_gaps: call bh_eval_set_observations first (it tells the plan the set of every chain)");
    if (nsets != p->nsets)
        return bh::fail_arg_(("bh_eval_set_gaps: nsets = " + std::to_string(nsets) + ", but bh_eval_set_observations gave the plan " +
                              std::to_string(p->nsets) + " sets").c_str());
    std::vector<int> tables;
    bool any_gap = false;
    if (int rc = bh::like_gaps_derive("bh_eval_set_gaps", nsets, p->row, p->T, p->like.data(), set_present, tables, &any_gap))
        return rc;
    if (any_gap) {
        BH_HIP(hipSetDevice(p->dev));
        int *d = nullptr;
        if (int rc = upload(&d, tables.data(), tables.size())) {
            if (d) (void)hipFree(d);
            return rc;
        }
        p->gaps = d;
    }
    p->gaps_set = true;
    return BH_OK;
}

int bh_eval_set_ellipticity(bh_eval_plan *p, int nell, const bh_ell_target *ell)
{
    if (nell < 1 || nell > BH_MAX_TARGETS) return bh::fail_arg_("bh_eval_set_ellipticity: nell outside 1 .. BH_MAX_TARGETS");
    if (!ell) return bh::fail_arg_("bh_eval_set_ellipticity: NULL pointer (ell)");
    if (!p) return bh::fail_arg_("plan is NULL");
    if (p->submitted) return bh::fail_arg_("bh_eval_set_ellipticity: called after bh_eval_submit");
    if (!p->ell.empty()) return bh::fail_arg_("bh_eval_set_ellipticity: the plan has its ellipticity targets already");
    for (int i = 0; i < nell; i++) {
        const bh_ell_target &e = ell[i];
        const std::string who = "bh_eval_set_ellipticity: ell[" + std::to_string(i) + "].";
        if (e.src < 0 || e.src >= p->nswd)
            return bh::fail_arg_((who + "src = " + std::to_string(e.src) + " is outside the plan's " + std::to_string(p->nswd) +
                                  " dispersion targets").c_str());
        const bh_swd_target &s = p->swd[e.src];
        if (s.iwave != 2 || s.igr != 0 || s.mode != 1)
            return bh::fail_arg_((who + "src names a target that is not the fundamental Rayleigh mode's phase velocity "
                                  "(iwave 2, igr 0, mode 1)").c_str());
        if (e.nper < 1 || e.nper > BH_MAX_PERIODS || e.nper != s.nper)
            return bh::fail_arg_((who + "nper = " + std::to_string(e.nper) + ": 1 .. 60 and the source's (" +
                                  std::to_string(s.nper) + ")").c_str());
        if (e.out_off < 0 || e.out_off + e.nper > p->row)
            return bh::fail_arg_((who + "out_off: the columns lie outside the row").c_str());
    }
    p->ell.assign(ell, ell + nell);
    return BH_OK;
}

int bh_eval_set_concurrency(bh_eval_plan *p, int plans_in_flight)
{
    if (!p || plans_in_flight < 1) return bh::fail_arg_("bh_eval_set_concurrency: bad argument");
    p->concurrency = plans_in_flight;
    return BH_OK;
}

int bh_eval_wait(bh_eval_plan *p, int *count)
{
    if (!p) return bh::fail_arg_("plan is NULL");
    if (p->failed) {
        if (count) *count = 0;
        return bh::fail_arg_(("the last bh_eval_submit of this plan failed: " + p->failure).c_str());
    }
    if (p->last_count > 0) BH_HIP(hipEventSynchronize(p->done));
    if (count) *count = p->last_count;
    return BH_OK;
}

}  // extern "C"
