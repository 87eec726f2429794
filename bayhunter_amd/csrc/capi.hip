// capi.hip -- the C ABI of libbayhunter_amd.so (include/bayhunter_amd.h): errors and the device check, the per-thread
// scratch, the order keys and the Voronoi kernel, the single-model dispersion drop-ins, the self-tests and the plumbing
// (malloc, memcpy, streams).  The dispersion launch path is in swd_launch.hip, the receiver-function entry points in
// rf_capi.hip, the likelihood's in like_capi.hip.  Host code only.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <string>
#include <vector>
#include "host_common.h"
#include "kernels.h"
#include "math_probe.h"

using bh::fail_arg_;
using bh::fail_hip_;

namespace {
thread_local std::string g_err;
}

int bh::fail_(int code, const char *what)
{
    g_err = what;
    return code;
}
int bh::fail_arg_(const char *what) { return fail_(BH_ERR_ARG, what); }
int bh::fail_hip_(int e, const char *what)
{
    g_err = std::string(what) + ": " + hipGetErrorString((hipError_t)e);
    return BH_ERR_HIP;
}

// HIP is initialised lazily on first use, never at load time: the reference forks one process per
// chain (mcmcOptimizer.py:248-252) and a HIP context must not be created before that fork.
int bh::require_device()
{
    static thread_local int ok = 0;
    if (ok) return BH_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail_(BH_ERR_NO_DEVICE, "no usable HIP device (libbayhunter_amd has no CPU fallback)");
    ok = 1;
    return BH_OK;
}

thread_local bh::Scratch bh::g_scratch;
int bh::Scratch::ensure(size_t bytes)
{
    int cur = 0;
    BH_HIP(hipGetDevice(&cur));
    if (cur != dev) { p = nullptr; n = 0; dev = cur; }   // buffer of another device: leave it be
    if (bytes <= n) return BH_OK;
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
    BH_HIP(hipMalloc(&p, bytes));
    n = bytes;
    return BH_OK;
}

extern "C" {

#ifndef BH_SRC_HASH
#define BH_SRC_HASH "unknown"
#endif
const char *bh_version(void) { return "bayhunter_amd 0.2 (gfx950) src " BH_SRC_HASH; }
const char *bh_last_error(void) { return g_err.c_str(); }

int bh_device_count(int *count)
{
    if (!count) return fail_arg_("count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess) ? n : 0;
    return BH_OK;
}

int bh_set_device(int device)
{
    int rc = bh::require_device();
    if (rc) return rc;
    BH_HIP(hipSetDevice(device));
    return BH_OK;
}

int bh_swd_order_keys(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vs,
                      double longest_period, int by_length, int *keys, void *stream)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return fail_arg_("model_stride < Lmax");
    if (B == 0) return BH_OK;
    if (!nlay || !h || !vs || !keys) return fail_arg_("NULL pointer");
    if (!(longest_period > 0)) return fail_arg_("longest_period must be positive");
    int rc = bh::require_device();
    if (rc) return rc;
    BH_HIP(bh::launch_order_keys(B, Lmax, model_stride, nlay, h, vs, 0.35 * 3.5 * longest_period, by_length, keys,
                                 (hipStream_t)stream));
    return BH_OK;
}

int bh_voronoi_to_layers(int B, int Lmax, const int *nlay, const double *vs_nuclei,
                         const double *z_nuclei, const double *vpvs, const bh_model_priors *pri,
                         double *model, int *valid, void *stream)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail_arg_("B/Lmax out of range");
    if (B == 0) return BH_OK;
    if (!nlay || !vs_nuclei || !z_nuclei || !vpvs || !pri || !model || !valid) return fail_arg_("NULL pointer");
    int rc = bh::require_device();
    if (rc) return rc;
    bh::VoronoiArgs A;
    A.B = B; A.Lmax = Lmax; A.nlay = nlay; A.vs = vs_nuclei; A.z = z_nuclei; A.vpvs = vpvs;
    A.model = model; A.valid = valid;
    A.pri = bh::ModelPriorsDev{pri->layers_min, pri->layers_max, pri->vs_min, pri->vs_max, pri->z_min,
                               pri->z_max, pri->thickmin, pri->lowvelperc, pri->highvelperc,
                               pri->mantle_vs, pri->mantle_vpvs};
    BH_HIP(bh::launch_voronoi(A, (hipStream_t)stream));
    return BH_OK;
}

// ---- single-model drop-ins ------------------------------------------------------------------

int bh_surfdisp96(const float *thkm, const float *vpm, const float *vsm, const float *rhom,
                  int nlayer, int iflsph, int iwave, int mode, int igr, int kmax, const double *t,
                  double *cg, int *err)
{
    if (!thkm || !vpm || !vsm || !rhom || !t || !cg || !err) return fail_arg_("NULL pointer");
    if (nlayer < 1 || nlayer > BH_MAX_LAYERS) return fail_arg_("nlayer out of range (max 100)");
    if (kmax < 0 || kmax > BH_MAX_PERIODS) return fail_arg_("kmax out of range (max 60)");
    int rc = bh::require_device();
    if (rc) return rc;
    const int L = nlayer;
    // host staging: [h|vp|vs|rho] fp64 (exactly representable fp32 values), periods, nlay
    std::vector<double> hb(4 * (size_t)L + BH_MAX_PERIODS);
    for (int i = 0; i < L; i++) {
        hb[i] = thkm[i]; hb[L + i] = vpm[i]; hb[2 * L + i] = vsm[i]; hb[3 * L + i] = rhom[i];
    }
    for (int k = 0; k < kmax; k++) hb[4 * L + k] = t[k];
    size_t off_out = hb.size() * sizeof(double);
    size_t off_ws = off_out + BH_MAX_PERIODS * sizeof(double);
    size_t off_int = off_ws + 2 * BH_MAX_PERIODS * sizeof(double);
    size_t total = off_int + 2 * sizeof(int);
    rc = bh::g_scratch.ensure(total);
    if (rc) return rc;
    char *d = (char *)bh::g_scratch.p;
    BH_HIP(hipMemcpy(d, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice));
    int ints[2] = {nlayer, 0};
    BH_HIP(hipMemcpy(d + off_int, ints, sizeof(ints), hipMemcpyHostToDevice));
    bh_swd_target tg = {iwave, igr, mode, iflsph, kmax, 0, 0, 0};
    const double *dm = (const double *)d;
    rc = bh_swd_batch(1, L, L, (const int *)(d + off_int), dm, dm + L, dm + 2 * L, dm + 3 * L, 1, &tg,
                      dm + 4 * L, (double *)(d + off_out), BH_MAX_PERIODS, (int *)(d + off_int) + 1,
                      d + off_ws, 2 * BH_MAX_PERIODS * sizeof(double), nullptr);
    if (rc) return rc;
    BH_HIP(hipDeviceSynchronize());
    if (kmax > 0) BH_HIP(hipMemcpy(cg, d + off_out, kmax * sizeof(double), hipMemcpyDeviceToHost));
    BH_HIP(hipMemcpy(err, (int *)(d + off_int) + 1, sizeof(int), hipMemcpyDeviceToHost));
    return BH_OK;
}

// ---- the reference's own FFI symbols ------------------------------------------------------------
// What f2py binds for `subroutine surfdisp96` (surfdisp96.f:55-56: every argument by reference, no
// return value) and what rfmini.pyx:74-114 binds (wrap.cpp:57-63: returns 1).  Neither has an error
// channel beyond `err`: when the library itself fails (no device, limits) the message goes to stderr
// and the caller sees the reference's failure convention -- err != 0 (SurfDisp.run_model then returns
// (nan, nan), surf96_modsw.py:119-126) or a NaN trace (rejected by Targets.py:204-214).
void surfdisp96_(const float *thkm, const float *vpm, const float *vsm, const float *rhom,
                 const int *nlayer, const int *iflsph, const int *iwave, const int *mode, const int *igr,
                 const int *kmax, const double *t, double *cg, int *err)
{
    int rc = (nlayer && iflsph && iwave && mode && igr && kmax && err)
                 ? bh_surfdisp96(thkm, vpm, vsm, rhom, *nlayer, *iflsph, *iwave, *mode, *igr, *kmax, t, cg, err)
                 : fail_arg_("NULL pointer");
    if (rc != BH_OK) {
        std::fprintf(stderr, "libbayhunter_amd: surfdisp96_ failed (%d): %s\n", rc, g_err.c_str());
        if (err) *err = 100 + rc;
    }
}

int bh_selftest_division(long n, unsigned seed, int max_exp, long *mismatches)
{
    if (!mismatches || n < 0 || max_exp < 0 || max_exp > 500) return fail_arg_("bad argument");
    int rc = bh::require_device();
    if (rc) return rc;
    unsigned long long *d = nullptr, h = 0;
    BH_HIP(hipMalloc((void **)&d, sizeof(h)));
    BH_HIP(hipMemset(d, 0, sizeof(h)));
    BH_HIP(bh::launch_division_selftest(n, seed, max_exp, d, nullptr));
    BH_HIP(hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost));
    BH_HIP(hipFree(d));
    *mismatches = (long)h;
    return BH_OK;
}

// One primitive of math_probe.h over n elements.  The device buffers cover whole workgroups and the input's tail behind
// element n is NaN (all bits set), so a kernel that lost its `i < n` guard would stay inside its allocations and
// rf_cexp_pair's wave-uniform test would see lanes outside its bound there.
int bh_selftest_math(int op, long n, const double *in, double *out)
{
    if (op < 0 || op >= bh::MP_NOPS) return fail_arg_("unknown op");
    if (n < 0 || n > (1L << 28)) return fail_arg_("n out of range");
    if (!in || !out) return fail_arg_("NULL pointer");
    int rc = bh::require_device();
    if (rc) return rc;
    if (n == 0) return BH_OK;
    const size_t npad = ((size_t)n + 255) / 256 * 256;
    const size_t bin = npad * bh::MP_IN * sizeof(double), bout = npad * bh::MP_OUT * sizeof(double);
    const size_t nin = (size_t)n * bh::MP_IN * sizeof(double), nout = (size_t)n * bh::MP_OUT * sizeof(double);
    char *d = nullptr;
    BH_HIP(hipMalloc((void **)&d, bin + bout));
    hipError_t e = hipMemset(d, 0xff, bin + bout);
    if (e == hipSuccess) e = hipMemcpy(d, in, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = bh::launch_math_probe(op, n, (const double *)d, (double *)(d + bin), nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + bin, nout, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    BH_HIP(e);
    return BH_OK;
}

// ---- plumbing ----------------------------------------------------------------------------------
int bh_malloc(void **dptr, size_t bytes)
{
    if (!dptr) return fail_arg_("dptr is NULL");
    int rc = bh::require_device();
    if (rc) return rc;
    BH_HIP(hipMalloc(dptr, bytes));
    return BH_OK;
}
int bh_free(void *dptr)
{
    BH_HIP(hipFree(dptr));
    return BH_OK;
}
int bh_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream)
{
    BH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return BH_OK;
}
int bh_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream)
{
    BH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return BH_OK;
}
int bh_stream_synchronize(void *stream)
{
    BH_HIP(hipStreamSynchronize((hipStream_t)stream));
    return BH_OK;
}
int bh_stream_create(void **stream)
{
    if (!stream) return fail_arg_("stream is NULL");
    int rc = bh::require_device();
    if (rc) return rc;
    hipStream_t s = nullptr;
    BH_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return BH_OK;
}
int bh_stream_destroy(void *stream)
{
    if (!stream) return fail_arg_("the null stream cannot be destroyed");
    int rc = bh_stream_retire(stream);
    if (rc) return rc;
    BH_HIP(hipStreamDestroy((hipStream_t)stream));
    return BH_OK;
}

}  // extern "C"
