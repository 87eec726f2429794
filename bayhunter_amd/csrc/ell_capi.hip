// ell_capi.hip -- the C ABI of the Rayleigh-wave ellipticity (include/bayhunter_amd.h): bh_ell_batch and
// bh_ell_batch_rows on device pointers and the synchronous single-model drop-in bh_ellipticity.  Host code only; the
// kernels are in ellipticity.hip and ell_rows.hip.
#include <hip/hip_runtime.h>
#include <vector>
#include "ell_launch.h"
#include "host_common.h"

extern "C" {

int bh_ell_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp, const double *vs,
                 const double *rho, int nper, const double *periods, int flsph, const double *c, int c_stride,
                 const int *c_err, int err_stride, int absolute, double *out, int out_stride, void *stream)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return bh::fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return bh::fail_arg_("model_stride < Lmax");
    if (nper < 1 || nper > BH_MAX_PERIODS) return bh::fail_arg_("nper out of range (1 .. 60)");
    if (c_stride < nper || out_stride < nper) return bh::fail_arg_("c_stride / out_stride shorter than nper");
    if (err_stride < 1) return bh::fail_arg_("err_stride < 1");
    if (!nlay || !h || !vp || !vs || !rho || !periods || !c || !c_err || !out) return bh::fail_arg_("NULL pointer");
    if (B == 0) return BH_OK;
    int rc = bh::require_device();
    if (rc) return rc;
    bh::EllArgs A;
    A.B = B; A.Lmax = Lmax; A.nper = nper; A.mstride = model_stride;
    A.flsph = flsph == 1; A.absolute = absolute != 0;
    A.c_stride = c_stride; A.err_stride = err_stride; A.out_stride = out_stride;
    A.nlay = nlay; A.h = h; A.vp = vp; A.vs = vs; A.rho = rho;
    A.periods = periods; A.c = c; A.c_err = c_err; A.out = out;
    BH_HIP(bh::launch_ell(A, (hipStream_t)stream));
    return BH_OK;
}

int bh_ell_batch_rows(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp,
                      const double *vs, const double *rho, int nper, const double *periods, int flsph, const double *c,
                      int c_stride, int *err, int err_stride, int absolute, double *out, int out_stride, const int *order,
                      int raise_flag, void *stream)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return bh::fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return bh::fail_arg_("model_stride < Lmax");
    if (nper < 1 || nper > BH_MAX_PERIODS) return bh::fail_arg_("nper out of range (1 .. 60)");
    if (c_stride < nper || out_stride < nper) return bh::fail_arg_("c_stride / out_stride shorter than nper");
    if (err_stride < 1) return bh::fail_arg_("err_stride < 1");
    if (!nlay || !h || !vp || !vs || !rho || !periods || !c || !err || !out) return bh::fail_arg_("NULL pointer");
    if (B == 0) return BH_OK;
    int rc = bh::require_device();
    if (rc) return rc;
    bh::EllRowsArgs A;
    A.B = B; A.Lmax = Lmax; A.nper = nper; A.mstride = model_stride;
    A.flsph = flsph == 1; A.absolute = absolute != 0;
    A.c_stride = c_stride; A.err_stride = err_stride; A.out_stride = out_stride;
    A.raise_flag = raise_flag != 0;
    A.nlay = nlay; A.h = h; A.vp = vp; A.vs = vs; A.rho = rho;
    A.periods = periods; A.c = c; A.order = order; A.err = err; A.out = out;
    BH_HIP(bh::launch_ell_rows(A, (hipStream_t)stream));
    return BH_OK;
}

int bh_ellipticity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer, int iflsph,
                   int kmax, const double *t, int absolute, double *ell, int *err)
{
    if (!thkm || !vpm || !vsm || !rhom || !t || !ell || !err) return bh::fail_arg_("NULL pointer");
    if (nlayer < 1 || nlayer > BH_MAX_LAYERS) return bh::fail_arg_("nlayer out of range (max 100)");
    if (kmax < 1 || kmax > BH_MAX_PERIODS) return bh::fail_arg_("kmax out of range (1 .. 60)");
    // the search: fundamental-mode Rayleigh phase velocities, through the dispersion drop-in
    std::vector<double> cg(kmax);
    int rc = bh_surfdisp96(thkm, vpm, vsm, rhom, nlayer, iflsph, 2, 1, 0, kmax, t, cg.data(), err);
    if (rc) return rc;
    // the pass: [h|vp|vs|rho|t|c] fp64 (exactly representable fp32 layers), then the output row and [nlay, err]
    const int L = nlayer;
    std::vector<double> hb(4 * (size_t)L + 2 * (size_t)kmax);
    for (int i = 0; i < L; i++) {
        hb[i] = thkm[i]; hb[L + i] = vpm[i]; hb[2 * L + i] = vsm[i]; hb[3 * L + i] = rhom[i];
    }
    for (int k = 0; k < kmax; k++) { hb[4 * L + k] = t[k]; hb[4 * L + kmax + k] = cg[k]; }
    const size_t off_out = hb.size() * sizeof(double);
    const size_t off_int = off_out + kmax * sizeof(double);
    rc = bh::g_scratch.ensure(off_int + 2 * sizeof(int));
    if (rc) return rc;
    char *d = (char *)bh::g_scratch.p;
    BH_HIP(hipMemcpy(d, hb.data(), off_out, hipMemcpyHostToDevice));
    const int ints[2] = {nlayer, *err};
    BH_HIP(hipMemcpy(d + off_int, ints, sizeof(ints), hipMemcpyHostToDevice));
    const double *dm = (const double *)d;
    rc = bh_ell_batch(1, L, L, (const int *)(d + off_int), dm, dm + L, dm + 2 * L, dm + 3 * L, kmax, dm + 4 * L, iflsph,
                      dm + 4 * L + kmax, kmax, (const int *)(d + off_int) + 1, 1, absolute, (double *)(d + off_out), kmax,
                      nullptr);
    if (rc) return rc;
    BH_HIP(hipDeviceSynchronize());
    BH_HIP(hipMemcpy(ell, d + off_out, kmax * sizeof(double), hipMemcpyDeviceToHost));
    return BH_OK;
}

}  // extern "C"
