// CPU replay of rf_kernel as it runs since the bounded attenuation exponent and the radix-4 passes: rf_host.h's
// rf_host_replay (phases 1-4 of one model: the phase functions of rf_core.h, the transform's plan and butterflies the
// kernel uses), and probes of the two forms of the exponential.  Built by tests/test_rf_floor.py with the device math of
// bh_math.h (the flags of conftest's hostsim_devmath build).
#define BH_HOSTSIM 1
#include <cmath>
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/rf_host.h"

using namespace bh;

// radix4 = 0: every stage of the transform as a radix-2 stage (the transform before the radix-4 passes)
extern "C" void hs_rf_floor(int nlay, const double *h, const double *vp, const double *vs, const double *rho,
                            const double *qp, const double *qs, double p, double gauss, int nsamp, double fsamp,
                            double tshift, double nsv, int waveno, int nout, double *rf, int radix4)
{
    const RfLayout lo = rf_layout(nlay, nsamp);
    std::vector<double> S(lo.per_model), tw(2 * (size_t)nsamp), ftab((size_t)RF_FTAB * (nsamp / 2 + 1));
    rf_host_replay(nlay, h, vp, vs, rho, qp, qs, p, gauss, nsamp, fsamp, tshift, nsv, waveno, nout, S.data(), tw.data(),
                   ftab.data(), rf, radix4 != 0);
}

// the exponent without range reduction and the full form, and the bound below which the kernel takes the first
extern "C" double hs_exp_forms(int n, const double *x, double *small, double *full)
{
    for (int i = 0; i < n; i++) {
        small[i] = rf_exp_small(x[i]);
        full[i] = bh_exp_bounded(x[i]);
    }
    return RF_EXP_SMALL;
}

// rf_cexp_pair as phase 3 calls it, one virtual thread at a time: [n][4] = re, im of the two phase factors
extern "C" void hs_cexp_pair(int n, const double *za, const double *zb, double *out)
{
    for (int i = 0; i < n; i++) {
        cd ea, eb;
        rf_cexp_pair(mk(za[2 * i], za[2 * i + 1]), mk(zb[2 * i], zb[2 * i + 1]), &ea, &eb);
        out[4 * i] = ea.re; out[4 * i + 1] = ea.im; out[4 * i + 2] = eb.re; out[4 * i + 3] = eb.im;
    }
}

// cexp_bounded of one argument: the phase factor as the parent of the bounded form computed it
extern "C" void hs_cexp_full(int n, const double *z, double *out)
{
    for (int i = 0; i < n; i++) {
        const cd e = cexp_bounded(mk(z[2 * i], z[2 * i + 1]));
        out[2 * i] = e.re; out[2 * i + 1] = e.im;
    }
}
