// ell_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Host twin of ell_kernel (bayhunter_amd/csrc/ellipticity.hip): ell_core.h compiled with g++ and the device math of
// bh_math.h (the flags of conftest's hostsim_devmath build), one (model, period) at a time with the kernel's own
// conditions for a NaN.  Also the search that supplies c (swd_lane, as tests/hostsim/hostsim.cpp runs it), so that
// es_ellipticity is the twin of bh_ellipticity.  Never loaded by the bayhunter_amd package.
#define BH_HOSTSIM 1
#include <cmath>
#include <vector>
#include "../../bayhunter_amd/csrc/ell_core.h"

namespace {
struct HostLay {
    float *pd, *pa, *pb, *pr;
    float d(int i) const { return pd[i]; }
    float a(int i) const { return pa[i]; }
    float b(int i) const { return pb[i]; }
    float rho(int i) const { return pr[i]; }
    void set_d(int i, float v) { pd[i] = v; }
    void set_a(int i, float v) { pa[i] = v; }
    void set_b(int i, float v) { pb[i] = v; }
    void set_rho(int i, float v) { pr[i] = v; }
};
struct OneTask {
    HostLay src;
    int nlayer, taken = 0, err = -1;
    double *out, *cws, *cbws;
    int next(HostLay &lay, double *&o, double *&c, double *&cb)
    {
        if (taken) return 0;
        taken = 1;
        lay = src;
        o = out; c = cws; cb = cbws;
        return nlayer;
    }
    void done(int e) { err = e; }
    void sphere(HostLay &lay, int mmax, int ifunc) { bh::swd_sphere(lay, mmax, ifunc); }
    void put(bh::SwdState &S, int k, int kmax, float v) { bh::swd_put_direct(S, k, kmax, v); }
    void fill_zero(bh::SwdState &S, int k, int kmax) { bh::swd_zero_direct(S, k, kmax); }
};

template <int FORM>
double one_value(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int flsph, int path,
                 double t1, double c, bool absolute)
{
    const bh::EllModelLay m{h, vp, vs, rho};
    if (!flsph) return bh::ell_value_form<FORM>(m, nlay, t1, c, absolute);
    if (path == 0) return bh::ell_value_form<FORM>(bh::EllSphere<bh::EllModelLay>{m}, nlay, t1, c, absolute);
    // path 1: the model transformed once by swd_sphere, as the dispersion search sees it
    std::vector<float> d(nlay), a(nlay), b(nlay), r(nlay);
    for (int i = 0; i < nlay; i++) { d[i] = m.d(i); a[i] = m.a(i); b[i] = m.b(i); r[i] = m.rho(i); }
    HostLay lay{d.data(), a.data(), b.data(), r.data()};
    bh::swd_sphere(lay, nlay, 2);
    return bh::ell_value_form<FORM>(lay, nlay, t1, c, absolute);
}
}  // namespace

// One row of bh_ell_batch: out[k], k < nper.  h/vp/vs/rho fp64 with nlay valid entries (Lmax: the call's depth), c the
// row's phase velocities, err its flag.  form: 0 ELL_FORM_TZ (the library's), 1 ELL_FORM_TR.  sphere_path (flsph = 1):
// 0 the kernel's layer-by-layer transformation, 1 swd_sphere on a copy of the model.
extern "C" void es_ell_row(const double *h, const double *vp, const double *vs, const double *rho, int nlay, int Lmax,
                           int flsph, int nper, const double *t, const double *c, int err, int absolute, int form,
                           int sphere_path, double *out)
{
    const bool bad = err != 0 || nlay < 2 || nlay > Lmax;
    for (int k = 0; k < nper; k++) {
        if (bad) { out[k] = std::nan(""); continue; }
        out[k] = form == 0 ? one_value<bh::ELL_FORM_TZ>(h, vp, vs, rho, nlay, flsph, sphere_path, t[k], c[k], absolute != 0)
                           : one_value<bh::ELL_FORM_TR>(h, vp, vs, rho, nlay, flsph, sphere_path, t[k], c[k], absolute != 0);
    }
}

// Twin of bh_ellipticity: the fundamental-mode Rayleigh phase search of the model (real*4 layers), then the pass.
// cg [kmax] receives the phase velocities, the return value is the search's err flag.
extern "C" int es_ellipticity(const float *thkm, const float *vpm, const float *vsm, const float *rhom, int nlayer,
                              int iflsph, int kmax, const double *t, int absolute, double *ell, double *cg)
{
    std::vector<float> d(thkm, thkm + nlayer), a(vpm, vpm + nlayer), b(vsm, vsm + nlayer), r(rhom, rhom + nlayer);
    HostLay lay{nullptr, nullptr, nullptr, nullptr};
    bh::SwdTargetDev tg{2, 0, 1, iflsph, kmax, 0, 0, 0};
    std::vector<double> cws(kmax > 0 ? kmax : 1), cbws(kmax > 0 ? kmax : 1);
    OneTask src{HostLay{d.data(), a.data(), b.data(), r.data()}, nlayer, 0, -1, cg, cws.data(), cbws.data()};
    bh::swd_lane(lay, src, tg, t, 1, nullptr);
    std::vector<double> h(thkm, thkm + nlayer), vp(vpm, vpm + nlayer), vs(vsm, vsm + nlayer), rho(rhom, rhom + nlayer);
    es_ell_row(h.data(), vp.data(), vs.data(), rho.data(), nlayer, nlayer, iflsph, kmax, t, cg, src.err, absolute, 0, 0, ell);
    return src.err;
}
