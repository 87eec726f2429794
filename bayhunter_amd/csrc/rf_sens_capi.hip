// rf_sens_capi.hip -- the C ABI of the receiver-function sensitivity kernels (include/bayhunter_amd.h): bh_rf_sens_batch
// on device pointers and the synchronous single-model form bh_rf_sensitivity.  Host code only; the kernel is in
// rf_sens.hip.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "host_common.h"
#include "kernels.h"
#include "rf_host.h"
#include "rf_sens_core.h"

using bh::fail_arg_;

namespace {

// The checks both entry points share, then the launch.  sigma NaN: Poisson's ratio from each variant's top layer.
int rf_sens_launch_(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp, const double *vs,
                    const double *rho, const double *qp, const double *qs, const bh_rf_params *par, double sigma, double *K,
                    long long k_stride, void *stream)
{
    if (!par) return fail_arg_("par is NULL");
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return fail_arg_("model_stride < Lmax");
    bh_rf_params q = *par;
    q.out_off = 0;                                     // K and rf have rows of their own
    int rc = bh::check_rf_params(&q, Lmax, q.nout, false);
    if (rc) return rc;
    if (k_stride < (long long)q.nout * 4 * Lmax) return fail_arg_("k_stride shorter than nout * 4 * Lmax");
    if (!nlay || !h || !vp || !vs || !rho || !K) return fail_arg_("NULL pointer");
    if (B == 0) return BH_OK;
    const int pairs = bh::rf_sens_pairs(Lmax, q.nsamp);
    const long long chunks = (4 * Lmax - 1 + (pairs > 0 ? pairs : 1) - 1) / (pairs > 0 ? pairs : 1);
    if ((long long)B * chunks > 0x7fffffffLL) return fail_arg_("B * (4 * Lmax - 1) slots do not fit one launch");
    if ((rc = bh::require_device())) return rc;
    bh::RfSensArgs A;
    std::memset(&A, 0, sizeof(A));
    bh::rf_fill_launch(A.P, q.p, q.gauss, q.nsamp, q.fsamp, q.tshift, q.nsv, q.waveno, q.nout);
    A.P.sigma = sigma;
    A.P.Lmax = Lmax;
    A.P.out_stride = q.nout;
    A.P.M = 1;
    bh::RfTables tables;                               // held until the launch below has been queued
    rc = bh::rf_get_tables(A.P, q.fsamp, &tables);
    if (rc) return rc;
    A.tw = tables.tw; A.ftab = tables.ftab;
    A.B = B; A.mstride = model_stride; A.nlay = nlay; A.h = h; A.vp = vp; A.vs = vs; A.rho = rho; A.qp = qp; A.qs = qs;
    A.K = K; A.k_stride = (long)k_stride;
    A.st = bh::rf_sens_steps();
    BH_HIP(bh::launch_rf_sens(A, (hipStream_t)stream));
    return BH_OK;
}

}  // namespace

extern "C" {

size_t bh_rf_sens_workspace_bytes(int, int) { return 0; }      // the perturbed traces live in LDS

int bh_rf_sens_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp, const double *vs,
                     const double *rho, const double *qp, const double *qs, const bh_rf_params *par, double *K,
                     long long k_stride, double *rf, int rf_stride, void *, size_t, void *stream)
{
    if (par && rf && rf_stride < par->nout) return fail_arg_("rf_stride shorter than nout");
    int rc = rf_sens_launch_(B, Lmax, model_stride, nlay, h, vp, vs, rho, qp, qs, par, std::nan(""), K, k_stride, stream);
    if (rc || B == 0 || !rf) return rc;
    bh_rf_params q = *par;                             // the unperturbed trace: bh_rf_batch's own launch on the same rows
    q.out_off = 0;
    return bh_rf_batch(B, Lmax, model_stride, nlay, h, vp, vs, rho, qp, qs, &q, rf, rf_stride, nullptr, 0, stream);
}

int bh_rf_sensitivity(int nsamp, double fsamp, double tshift, double p, double a, double nsv, double sigma, int waveno,
                      int nlay, const double *z, const double *vp, const double *vs, const double *rh, const double *qp,
                      const double *qs, double *fz, double *fr, double *rf, double *K)
{
    if (!K) return fail_arg_("NULL pointer");
    // the unperturbed trace (and bh_synrf's argument checks): bh_synrf's bits
    int rc = bh_synrf(nsamp, fsamp, tshift, p, a, nsv, sigma, waveno, nlay, z, vp, vs, rh, qp, qs, fz, fr, rf);
    if (rc) return rc;
    const int L = nlay;
    std::vector<double> hb(6 * (size_t)L);
    for (int i = 0; i < L; i++) {                      // thicknesses from the layer tops; the half-space has none
        hb[i] = i < L - 1 ? z[i + 1] - z[i] : 0.0;
        hb[L + i] = vp[i]; hb[2 * L + i] = vs[i]; hb[3 * L + i] = rh[i]; hb[4 * L + i] = qp[i]; hb[5 * L + i] = qs[i];
    }
    const size_t nK = (size_t)nsamp * 4 * L;
    const size_t off_K = hb.size() * sizeof(double), off_int = off_K + nK * sizeof(double);
    rc = bh::g_scratch.ensure(off_int + sizeof(int));
    if (rc) return rc;
    char *d = (char *)bh::g_scratch.p;
    BH_HIP(hipMemcpy(d, hb.data(), off_K, hipMemcpyHostToDevice));
    BH_HIP(hipMemcpy(d + off_int, &nlay, sizeof(int), hipMemcpyHostToDevice));
    bh_rf_params par;
    std::memset(&par, 0, sizeof(par));
    par.p = p; par.gauss = a; par.fsamp = fsamp; par.tshift = tshift; par.nsv = nsv;
    par.nsamp = nsamp; par.waveno = waveno; par.nout = nsamp; par.out_off = 0;
    const double *dm = (const double *)d;
    rc = rf_sens_launch_(1, L, L, (const int *)(d + off_int), dm, dm + L, dm + 2 * L, dm + 3 * L, dm + 4 * L, dm + 5 * L, &par,
                         sigma, (double *)(d + off_K), (long long)nK, nullptr);
    if (rc) return rc;
    BH_HIP(hipDeviceSynchronize());
    BH_HIP(hipMemcpy(K, d + off_K, nK * sizeof(double), hipMemcpyDeviceToHost));
    return BH_OK;
}

}  // extern "C"
