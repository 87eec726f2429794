// rf_capi.hip -- the receiver-function entry points of the C ABI (include/bayhunter_amd.h) and the two table caches
// their launches read.  Host code only.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include "host_common.h"
#include "kernels.h"
#include "rf_host.h"

using bh::fail_arg_;
using bh::fail_hip_;

namespace {

// FFT twiddle tables, one per (device, nsamp), built on the host like fork.cpp:50-51.
std::mutex g_rf_tables_mutex;          // guards both caches: g_tw, and g_ftab with its clock and pins
std::map<std::pair<int, int>, double *> g_tw;

int get_twiddles(int nsamp, const double **out)
{
    int dev = 0;
    BH_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_rf_tables_mutex);
    auto key = std::make_pair(dev, nsamp);
    auto it = g_tw.find(key);
    if (it == g_tw.end()) {
        std::vector<double> tw(2 * (size_t)nsamp);
        bh::rf_fill_twiddles(tw.data(), nsamp);
        double *d = nullptr;
        BH_HIP(hipMalloc((void **)&d, tw.size() * sizeof(double)));
        BH_HIP(hipMemcpy(d, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
        it = g_tw.emplace(key, d).first;
    }
    *out = it->second;
    return BH_OK;
}

// Per-frequency constants of the receiver-function kernel (rf_host.h, rf_fill_freq_table): one table per
// (device, nsamp, fsamp, gauss, tshift), built on the host with the reference's expressions.  A run uses a
// handful of parameter sets, but a caller of the single-model drop-ins may vary the Gauss width or the time
// shift per call (a sweep of 24 585 configurations did), so the cache is bounded: beyond kFtabMax tables the
// least recently used one that no call holds goes.  A table is pinned from the look-up to the launch; hipFree
// waits for the device, so a launch that was started with the table has finished when it is released.
constexpr size_t kFtabMax = 64;
struct FreqTable { double *d = nullptr; unsigned long stamp = 0; int pins = 0; };
using FreqKey = std::tuple<int, int, double, double, double>;
std::map<FreqKey, FreqTable> g_ftab;
unsigned long g_ftab_clock = 0;

struct FreqTablePin {               // releases the pin when the call that looked the table up is done with it
    FreqTable *t = nullptr;
    ~FreqTablePin()
    {
        if (!t) return;
        std::lock_guard<std::mutex> lock(g_rf_tables_mutex);
        t->pins--;
    }
};

int get_freq_table(const bh::RfLaunch &P, double fsamp, const double **out, FreqTablePin *pin)
{
    int dev = 0;
    BH_HIP(hipGetDevice(&dev));
    const FreqKey key = std::make_tuple(dev, P.nsamp, fsamp, P.gauss, P.tshift);
    std::vector<double> tab;
    {
        std::lock_guard<std::mutex> lock(g_rf_tables_mutex);
        auto it = g_ftab.find(key);
        if (it != g_ftab.end()) {
            it->second.stamp = ++g_ftab_clock;
            it->second.pins++;
            pin->t = &it->second;                 // (std::map: the address of a value is stable)
            *out = it->second.d;
            return BH_OK;
        }
    }
    // not cached: table and upload outside the lock (two threads may both build one; the second is dropped)
    tab.resize((size_t)bh::RF_FTAB * P.nfreq);
    bh::rf_fill_freq_table(P, tab.data());
    double *d = nullptr;
    BH_HIP(hipMalloc((void **)&d, tab.size() * sizeof(double)));
    hipError_t ce = hipMemcpy(d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    if (ce != hipSuccess) { (void)hipFree(d); return fail_hip_((int)ce, "hipMemcpy(frequency table)"); }
    std::vector<double *> evicted;
    {
        std::lock_guard<std::mutex> lock(g_rf_tables_mutex);
        auto ins = g_ftab.emplace(key, FreqTable{});
        if (ins.second) ins.first->second.d = d; else evicted.push_back(d);
        ins.first->second.stamp = ++g_ftab_clock;
        ins.first->second.pins++;
        pin->t = &ins.first->second;
        *out = ins.first->second.d;
        while (g_ftab.size() > kFtabMax) {
            auto victim = g_ftab.end();
            for (auto jt = g_ftab.begin(); jt != g_ftab.end(); ++jt)
                if (jt->second.pins == 0 && (victim == g_ftab.end() || jt->second.stamp < victim->second.stamp)) victim = jt;
            if (victim == g_ftab.end()) break;    // every table is held by a call in progress
            evicted.push_back(victim->second.d);
            g_ftab.erase(victim);
        }
    }
    for (double *e : evicted) (void)hipFree(e);   // (synchronises with the device)
    return BH_OK;
}

int pick_rf_M(int B, int Lmax, int nsamp)
{
    // Models per workgroup.  rf_kernel is built for four waves per SIMD (128 VGPRs), so that one of its
    // workgroups fits next to the two 192-VGPR waves per SIMD of swd_kernel (2 x 192 + 128 = 512) and the two
    // kernels of a joint evaluation share the CUs from the start instead of running one after the other; the LDS
    // has to allow it too: eight swd_kernel waves hold 8 x 15.7 KiB of a CU's 160 KiB (ten layers, 21 periods),
    // which leaves ~31 KiB -- three 512-sample models.  Alone, four such workgroups per CU (98 KiB) keep all
    // four waves per SIMD resident.  (Six models per workgroup, the round-2 choice, is 1 % faster alone -- no
    // partial last round of tasks -- and can never be co-resident: 65.1 -> 61.2 ms per joint step, same box,
    // profiles/r03_ab_rf_coresident.txt.)
    size_t per = bh::rf_lds_bytes(Lmax, nsamp, 1);
    int M = (int)((26 * 1024) / per);
    if (M > 8) M = 8;
    if (M < 1) M = 1;
    if (M > B) M = B;
    return M;
}

int rf_launch_common(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp,
                     const double *vs, const double *rho, const double *qp, const double *qs,
                     const bh_rf_params *par, double sigma, int depth_input, double *out,
                     int out_stride, void *stream, double *out_fz = nullptr,
                     double *out_fr = nullptr, const double *set_p = nullptr, const int *set_id = nullptr,
                     int nsets = 0)
{
    if (!par) return fail_arg_("par is NULL");
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail_arg_("B/Lmax out of range");
    if (model_stride < Lmax) return fail_arg_("model_stride < Lmax");
    if (B == 0) return BH_OK;
    if (!nlay || !h || !vp || !vs || !rho || !out) return fail_arg_("NULL pointer");
    int rc = bh::check_rf_params(par, Lmax, out_stride, out_fz && out_fr);
    if (rc || (rc = bh::require_device())) return rc;
    const int n = par->nsamp;
    bh::RfArgs A;
    std::memset(&A, 0, sizeof(A));
    bh::rf_fill_launch(A.P, par->p, par->gauss, n, par->fsamp, par->tshift, par->nsv, par->waveno, par->nout);
    A.P.sigma = sigma;
    A.P.out_off = par->out_off;
    A.P.out_stride = out_stride;
    A.P.Lmax = Lmax;
    A.P.depth_input = depth_input;
    A.P.M = (out_fz && out_fr) ? 1 : pick_rf_M(B, Lmax, n);
    A.out_fz = out_fz; A.out_fr = out_fr;
    A.set_p = set_p; A.set_id = set_id; A.nsets = nsets;   // per-row slowness (bh_rf_batch_sets), or null / 0
    rc = get_twiddles(n, &A.tw);
    if (rc) return rc;
    FreqTablePin pin;                              // held until the launch below has been queued
    rc = get_freq_table(A.P, par->fsamp, &A.ftab, &pin);
    if (rc) return rc;
    A.B = B; A.mstride = model_stride; A.nlay = nlay; A.h = h; A.vp = vp; A.vs = vs; A.rho = rho; A.qp = qp; A.qs = qs;
    A.out = out;
    BH_HIP(bh::launch_rf(A, (hipStream_t)stream));
    return BH_OK;
}

}  // namespace

int bh::check_rf_params(const bh_rf_params *par, int Lmax, int out_stride, bool zr)
{
    const int n = par->nsamp;
    if (n < 8 || n > 4096 || (n & (n - 1))) return fail_arg_("nsamp must be a power of two in 8..4096");
    if (par->waveno != 0 && par->waveno != 1) return fail_arg_("waveno must be 0 (P) or 1 (SV)");
    if (par->nout < 1 || par->nout > n) return fail_arg_("nout out of range");
    if (par->out_off < 0 || par->out_off + par->nout > out_stride) return fail_arg_("RF does not fit the output row");
    if (!(par->gauss > 0) || !(par->fsamp > 0)) return fail_arg_("gauss and fsamp must be positive");
    if (rf_lds_bytes(Lmax, n, 1, zr) > kLdsLimit) return fail_arg_("model does not fit LDS");
    return BH_OK;
}

bh::RfTables::~RfTables() { delete (FreqTablePin *)pin; }

int bh::rf_get_tables(const bh::RfLaunch &P, double fsamp, bh::RfTables *tables)
{
    int rc = get_twiddles(P.nsamp, &tables->tw);
    if (rc) return rc;
    FreqTablePin *pin = new FreqTablePin;
    tables->pin = pin;
    return get_freq_table(P, fsamp, &tables->ftab, pin);
}

extern "C" {

size_t bh_rf_workspace_bytes(int, int, const bh_rf_params *) { return 0; }

int bh_rf_active_frequencies(const bh_rf_params *par)
{
    if (!par || par->nsamp < 8 || par->nsamp > 4096 || !(par->gauss > 0) || !(par->fsamp > 0)) return 0;
    bh::RfLaunch P;
    std::memset(&P, 0, sizeof(P));
    bh::rf_fill_launch(P, par->p, par->gauss, par->nsamp, par->fsamp, par->tshift, par->nsv, par->waveno, par->nout);
    return P.nact;
}

int bh_rf_batch(int B, int Lmax, int model_stride, const int *nlay, const double *h,
                const double *vp, const double *vs, const double *rho, const double *qp,
                const double *qs, const bh_rf_params *par, double *out, int out_stride, void *, size_t,
                void *stream)
{
    return rf_launch_common(B, Lmax, model_stride, nlay, h, vp, vs, rho, qp, qs, par, std::nan(""), 0,
                            out, out_stride, stream);
}

int bh_rf_batch_sets(int B, int Lmax, int model_stride, const int *nlay, const double *h, const double *vp,
                     const double *vs, const double *rho, const double *qp, const double *qs, const bh_rf_params *par,
                     int nsets, const double *set_p, const int *set_id, double *out, int out_stride, void *, size_t,
                     void *stream)
{
    if (nsets < 1) return fail_arg_("bh_rf_batch_sets: nsets < 1");
    if (!set_p) return fail_arg_("bh_rf_batch_sets: set_p is NULL");
    if (nsets > 1 && !set_id) return fail_arg_("bh_rf_batch_sets: set_id is NULL but nsets > 1");
    if (!par) return fail_arg_("par is NULL");
    bh_rf_params q = *par;
    q.p = 0.0;                 // ignored: every row takes its set's
    return rf_launch_common(B, Lmax, model_stride, nlay, h, vp, vs, rho, qp, qs, &q, std::nan(""), 0, out, out_stride,
                            stream, nullptr, nullptr, set_p, set_id, nsets);
}

// ---- single-model drop-in (the dispersion one is bh_surfdisp96, capi.hip) ---------------------------------
int bh_synrf(int nsamp, double fsamp, double tshift, double p, double a, double nsv, double sigma,
             int waveno, int nlay, const double *z, const double *vp, const double *vs,
             const double *rh, const double *qp, const double *qs, double *fz, double *fr, double *rf)
{
    if (!z || !vp || !vs || !rh || !qp || !qs || !rf) return fail_arg_("NULL pointer");
    if ((fz == nullptr) != (fr == nullptr)) return fail_arg_("pass both fz and fr, or neither");
    if (nlay < 1 || nlay > BH_MAX_LAYERS) return fail_arg_("nlay out of range (max 100)");
    if (nsamp < 8 || nsamp > 4096) return fail_arg_("nsamp out of range");
    int rc = bh::require_device();
    if (rc) return rc;
    const int L = nlay;
    std::vector<double> hb(6 * (size_t)L);
    for (int i = 0; i < L; i++) {
        hb[i] = z[i]; hb[L + i] = vp[i]; hb[2 * L + i] = vs[i]; hb[3 * L + i] = rh[i];
        hb[4 * L + i] = qp[i]; hb[5 * L + i] = qs[i];
    }
    size_t off_out = hb.size() * sizeof(double);
    size_t off_zr = off_out + (size_t)nsamp * sizeof(double);
    size_t off_int = off_zr + 2 * (size_t)nsamp * sizeof(double);
    rc = bh::g_scratch.ensure(off_int + sizeof(int));
    if (rc) return rc;
    char *d = (char *)bh::g_scratch.p;
    BH_HIP(hipMemcpy(d, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice));
    BH_HIP(hipMemcpy(d + off_int, &nlay, sizeof(int), hipMemcpyHostToDevice));
    bh_rf_params par;
    std::memset(&par, 0, sizeof(par));
    par.p = p; par.gauss = a; par.fsamp = fsamp; par.tshift = tshift; par.nsv = nsv;
    par.nsamp = nsamp; par.waveno = waveno; par.nout = nsamp; par.out_off = 0;
    const double *dm = (const double *)d;
    rc = rf_launch_common(1, L, L, (const int *)(d + off_int), dm, dm + L, dm + 2 * L, dm + 3 * L,
                          dm + 4 * L, dm + 5 * L, &par, sigma, 1, (double *)(d + off_out), nsamp, nullptr,
                          fz ? (double *)(d + off_zr) : nullptr,
                          fz ? (double *)(d + off_zr) + nsamp : nullptr);
    if (rc) return rc;
    BH_HIP(hipDeviceSynchronize());
    BH_HIP(hipMemcpy(rf, d + off_out, (size_t)nsamp * sizeof(double), hipMemcpyDeviceToHost));
    if (fz) {
        BH_HIP(hipMemcpy(fz, d + off_zr, (size_t)nsamp * sizeof(double), hipMemcpyDeviceToHost));
        BH_HIP(hipMemcpy(fr, d + off_zr + (size_t)nsamp * sizeof(double), (size_t)nsamp * sizeof(double),
                         hipMemcpyDeviceToHost));
    }
    return BH_OK;
}

// What rfmini.pyx:74-114 binds (wrap.cpp:57-63: returns 1): the reference's own FFI symbol, with the failure
// convention described at surfdisp96_ (capi.hip) -- the message goes to stderr and the caller sees a NaN trace.
int synrf_cwrap(int nsamp, double fsamp, double tshift, double p, double a, double nsv, double sigma,
                int waveno, int nlay, double *z, double *vp, double *vs, double *rh, double *qp, double *qs,
                double *fz, double *fr, double *rf)
{
    int rc = bh_synrf(nsamp, fsamp, tshift, p, a, nsv, sigma, waveno, nlay, z, vp, vs, rh, qp, qs, fz, fr, rf);
    if (rc == BH_OK) return 1;
    std::fprintf(stderr, "libbayhunter_amd: synrf_cwrap failed (%d): %s\n", rc, bh_last_error());
    for (int i = 0; i < nsamp && nsamp <= 4096; i++) {
        if (rf) rf[i] = std::nan("");
        if (fz) fz[i] = std::nan("");
        if (fr) fr[i] = std::nan("");
    }
    return 0;
}

// The twiddle table as this library's host code builds it (rf_host.h: rf_fill_twiddles; get_twiddles uploads the same
// doubles).  No device work.  The values are glibc's, but which of its functions a compiler calls for std::exp(complex)
// is the compiler's choice, and two builds of rf_fill_twiddles need not agree in the last bit of every entry: a test
// that wants the device's bits takes the table from here.
int bh_rf_twiddles(int nsamp, double *tw)
{
    if (nsamp < 8 || nsamp > 4096 || (nsamp & (nsamp - 1))) return fail_arg_("nsamp must be a power of two in 8..4096");
    if (!tw) return fail_arg_("NULL pointer");
    bh::rf_fill_twiddles(tw, nsamp);
    return BH_OK;
}

// Phase 4 of rf_kernel alone (rf_probe.hip) on B half spectra, M per workgroup, with the launch constants of
// rf_fill_launch and the cached twiddle table that bh_rf_batch's launches use.  The output buffer is NaN (all bits set)
// where the kernel does not write.
int bh_selftest_rf_transform(int nsamp, int Lmax, int M, int B, int paired, const double *spec, int nout, double *out)
{
    if (nsamp < 8 || nsamp > 4096 || (nsamp & (nsamp - 1))) return fail_arg_("nsamp must be a power of two in 8..4096");
    if (Lmax < 1 || Lmax > BH_MAX_LAYERS) return fail_arg_("Lmax out of range");
    if (M < 1 || M > 8) return fail_arg_("M must be 1..8");
    if (B < 0 || B > (1 << 20)) return fail_arg_("B out of range");
    if (nout < 1 || nout > nsamp) return fail_arg_("nout out of range");
    if (!spec || !out) return fail_arg_("NULL pointer");
    if (bh::rf_lds_bytes(Lmax, nsamp, M, paired != 0) > bh::kLdsLimit) return fail_arg_("buffers do not fit LDS");
    int rc = bh::require_device();
    if (rc) return rc;
    if (B == 0) return BH_OK;
    bh::RfLaunch P = bh::RfLaunch();
    bh::rf_fill_launch(P, 0.0, 1.0, nsamp, 1.0, 0.0, -1.0, 0, nout);      // sc, qn, log2n, nfreq: all phase 4 reads
    P.Lmax = Lmax;
    P.M = M;
    const double *tw = nullptr;
    rc = get_twiddles(nsamp, &tw);
    if (rc) return rc;
    const size_t nch = paired ? 2 : 1;
    const size_t bin = (size_t)B * nch * P.nfreq * 2 * sizeof(double), bout = (size_t)B * nch * nout * sizeof(double);
    char *d = nullptr;
    BH_HIP(hipMalloc((void **)&d, bin + bout));
    hipError_t e = hipMemset(d + bin, 0xff, bout);
    if (e == hipSuccess) e = hipMemcpy(d, spec, bin, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = bh::launch_rf_probe(P, B, paired ? 1 : 0, (const double *)d, tw, (double *)(d + bin), nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + bin, bout, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    BH_HIP(e);
    return BH_OK;
}

int bh_rf_cached_tables(void)
{
    std::lock_guard<std::mutex> lock(g_rf_tables_mutex);
    return (int)g_ftab.size();
}

}  // extern "C"
