// sens_capi_common.h -- the host side the C ABI of the three sensitivity passes shares (sens_capi.hip,
// sens_group_capi.hip, ell_sens_capi.hip): the argument checks of the batch entry points and the staging of the
// synchronous single-model forms.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "sens_pass.h"
#include "host_common.h"

namespace bh {

inline size_t sens_pass_workspace_bytes(int B, int nper, int ws_per_period)
{
    if (B < 0 || nper < 0) return 0;
    return (size_t)B * (size_t)nper * ws_per_period * sizeof(double);
}

// The checks of a batch entry point, in the order and with the messages of the ABI, up to the device check; fills P.
// iwave: null for a pass without one.  outputs: the pass's further required pointers are all there.  workspace_need,
// workspace_msg: the pass's bh_*_workspace_bytes(B, nper) and its failure's text.  BH_OK with B == 0: nothing to launch.
inline int sens_pass_check(SensPassArgs &P, int B, int Lmax, int model_stride, const int *nlay, const double *h,
                           const double *vp, const double *vs, const double *rho, const int *iwave, int nper,
                           const double *periods, int flsph, const double *c, int c_stride, const int *c_err, int err_stride,
                           double *K, double *c_out, bool outputs, const void *workspace, size_t workspace_bytes,
                           size_t workspace_need, const char *workspace_msg)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return fail_arg_("model_stride < Lmax");
    if (iwave && *iwave != 1 && *iwave != 2) return fail_arg_("iwave is neither 1 (Love) nor 2 (Rayleigh)");
    if (nper < 1 || nper > BH_MAX_PERIODS) return fail_arg_("nper out of range (1 .. 60)");
    if (flsph != 0) return fail_arg_("flsph: sensitivity kernels are formed on a flat earth only");
    if (c_stride < nper) return fail_arg_("c_stride shorter than nper");
    if (err_stride < 1) return fail_arg_("err_stride < 1");
    if (!nlay || !h || !vp || !vs || !rho || !periods || !c || !c_err || !K || !c_out || !outputs)
        return fail_arg_("NULL pointer");
    if (B == 0) return BH_OK;
    if (!workspace || workspace_bytes < workspace_need) return fail_(BH_ERR_WORKSPACE, workspace_msg);
    P.B = B; P.Lmax = Lmax; P.nper = nper; P.mstride = model_stride;
    P.c_stride = c_stride; P.err_stride = err_stride;
    P.nlay = nlay; P.h = h; P.vp = vp; P.vs = vs; P.rho = rho;
    P.periods = periods; P.c = c; P.c_err = c_err;
    P.K = K; P.c_out = c_out;
    if (!sens_pass_fits(P)) return fail_arg_("B * nper * 4 * Lmax lanes do not fit one launch");
    return require_device();
}

// One model of a single-model form on the device, in g_scratch: [h|vp|vs|rho|t|c] fp64 (exactly representable fp32
// layers), then [3 kmax outputs | workspace | K | K_phase] and [nlay, err].  One layout for the three passes: the phase
// pass, which has two outputs and no K_phase, leaves the third output plane and the K_phase region unused, so
// bh_sensitivity asks g_scratch for about twice the bytes its own layout took (32 L kmax bytes more, 192 KB at the
// limits of 100 layers and 60 periods).
struct SensStaged {
    int L, kmax;
    const int *nlay, *err;
    const double *h, *vp, *vs, *rho, *t, *c;
    double *out[3];          // [kmax] each; out[0] is c_out
    double *ws;
    size_t ws_bytes;
    double *K, *K_phase;     // K_phase: null when the caller asked for none
};

// A single-model form: its argument checks, the search (bh_surfdisp96), the staging, batch(const SensStaged &) -- the
// pass's batch entry point on the staged pointers -- the synchronise and the copies back.  iwave: null for a pass
// without one (Rayleigh).  out: the nout (2 or 3) [kmax] results of the pass in the order of SensStaged::out.
// K_phase: null for none.
template <class Batch>
int sens_pass_single(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int iflsph,
                     const int *iwave, int kmax, const double *t, int ws_per_period, double *K, double *K_phase,
                     double *const *out, int nout, int *err, Batch batch)
{
    bool outputs = true;
    for (int i = 0; i < nout; i++) outputs = outputs && out[i];
    if (!thkm || !vpm || !vsm || !rhom || !t || !K || !outputs || !err) return fail_arg_("NULL pointer");
    if (nlayer < 1 || nlayer > BH_MAX_LAYERS) return fail_arg_("nlayer out of range (max 100)");
    if (kmax < 1 || kmax > BH_MAX_PERIODS) return fail_arg_("kmax out of range (1 .. 60)");
    if (iwave && *iwave != 1 && *iwave != 2) return fail_arg_("iwave is neither 1 (Love) nor 2 (Rayleigh)");
    if (iflsph != 0) return fail_arg_("iflsph: sensitivity kernels are formed on a flat earth only");
    // the search: fundamental-mode phase velocities, through the dispersion drop-in
    std::vector<double> cg(kmax);
    int rc = bh_surfdisp96(thkm, vpm, vsm, rhom, nlayer, 0, iwave ? *iwave : 2, 1, 0, kmax, t, cg.data(), err);
    if (rc) return rc;
    const int L = nlayer;
    std::vector<double> hb(4 * (size_t)L + 2 * (size_t)kmax);
    for (int i = 0; i < L; i++) {
        hb[i] = thkm[i]; hb[L + i] = vpm[i]; hb[2 * L + i] = vsm[i]; hb[3 * L + i] = rhom[i];
    }
    for (int k = 0; k < kmax; k++) { hb[4 * L + k] = t[k]; hb[4 * L + kmax + k] = cg[k]; }
    const size_t nK = (size_t)kmax * 4 * L, nws = (size_t)kmax * ws_per_period;
    const size_t off_out = hb.size() * sizeof(double);
    const size_t off_int = off_out + (3 * (size_t)kmax + nws + 2 * nK) * sizeof(double);
    rc = g_scratch.ensure(off_int + 2 * sizeof(int));
    if (rc) return rc;
    char *d = (char *)g_scratch.p;
    BH_HIP(hipMemcpy(d, hb.data(), off_out, hipMemcpyHostToDevice));
    const int ints[2] = {nlayer, *err};
    BH_HIP(hipMemcpy(d + off_int, ints, sizeof(ints), hipMemcpyHostToDevice));
    const double *dm = (const double *)d;
    double *dout = (double *)(d + off_out);
    SensStaged s;
    s.L = L; s.kmax = kmax;
    s.nlay = (const int *)(d + off_int); s.err = s.nlay + 1;
    s.h = dm; s.vp = dm + L; s.vs = dm + 2 * L; s.rho = dm + 3 * L; s.t = dm + 4 * L; s.c = dm + 4 * L + kmax;
    for (int i = 0; i < 3; i++) s.out[i] = dout + i * kmax;
    s.ws = dout + 3 * kmax; s.ws_bytes = nws * sizeof(double);
    s.K = s.ws + nws; s.K_phase = K_phase ? s.K + nK : nullptr;
    rc = batch(s);
    if (rc) return rc;
    BH_HIP(hipDeviceSynchronize());
    for (int i = 0; i < nout; i++) BH_HIP(hipMemcpy(out[i], s.out[i], kmax * sizeof(double), hipMemcpyDeviceToHost));
    BH_HIP(hipMemcpy(K, s.K, nK * sizeof(double), hipMemcpyDeviceToHost));
    if (K_phase) BH_HIP(hipMemcpy(K_phase, s.K_phase, nK * sizeof(double), hipMemcpyDeviceToHost));
    return BH_OK;
}

}  // namespace bh
