// CPU replay of the per-row form of rf_kernel (phases 1-3) for the M models of one workgroup, each at the ray
// parameter of its own set: the same phase functions, the same per-model LDS blocks and the same thread-to-(model,
// layer) and thread-to-(model, frequency) numbering as kernels.hip, on a host array.  Built by
// tests/test_station_slowness.py with glibc math (-DBH_HOSTSIM -DBH_HOSTSIM_GLIBC_MATH).
#define BH_HOSTSIM 1
#include <cmath>
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/rf_host.h"

using namespace bh;

// h, vp, vs, rho: [M][L]; set_id may be null (nsets == 1).  spec: [M][nfreq][2], zero behind nact; a model whose set
// index is out of range reports bad[m] = 1 (and its spectrum is NaN).  Returns nact.
extern "C" int hs_rf_sets_spectra(int M, int L, const int *nlay, const double *h, const double *vp, const double *vs,
                                  const double *rho, int nsets, const double *set_p, const int *set_id, double gauss,
                                  int nsamp, double fsamp, double tshift, double nsv, int waveno, int nout, double *spec,
                                  int *bad)
{
    RfLaunch P;
    std::memset(&P, 0, sizeof(P));
    rf_fill_launch(P, std::nan(""), gauss, nsamp, fsamp, tshift, nsv, waveno, nout);   // the launch's own p: never read
    P.sigma = std::nan("");
    P.Lmax = L;
    P.M = M;
    const RfLayout lo = rf_layout(L, nsamp);
    const int pm = lo.per_model;
    std::vector<double> S((size_t)M * pm, 0.0), ftab((size_t)RF_FTAB * P.nfreq);
    rf_fill_freq_table(P, ftab.data());
    for (int idx = 0; idx < M * L; idx++) {                       // P1
        const int m = idx / L, i = idx - m * L, nl = nlay[m];
        if (i < nl)
            rf_phase1_layer(S.data() + (long)m * pm, lo, nl, i, h + m * L, vp + m * L, vs + m * L, rho + m * L, nullptr,
                            nullptr, 0);
    }
    for (int idx = 0; idx < M * L; idx++) {                       // P2
        const int m = idx / L, i = idx - m * L, nl = nlay[m];
        if (i < nl) {
            bool bad_set;
            const double u = rf_row_slowness(set_p, set_id, nsets, m, &bad_set);
            bad[m] = bad_set ? 1 : 0;
            rf_phase2_interface_at<true>(S.data() + (long)m * pm, lo, P, nl, i, vp[m * L], vs[m * L], u, u * u);
        }
    }
    std::vector<cd> out((size_t)M * P.nfreq, mk(0., 0.));
    for (int task = 0; task < M * P.nact; task++) {               // P3, model-major
        const int m = task / P.nact, j = task - m * P.nact;
        out[(size_t)m * P.nfreq + j] = rf_phase3_task_at<true>(S.data() + (long)m * pm, lo, P, nlay[m], j,
                                                               rf_freq_load_lgw(ftab.data(), j), nullptr, nullptr,
                                                               ftab.data());
    }
    for (size_t k = 0; k < out.size(); k++) { spec[2 * k] = out[k].re; spec[2 * k + 1] = out[k].im; }
    return P.nact;
}

// The uniform form for one model at ray parameter p: what hostsim.cpp's hs_rf runs up to the spectrum.
extern "C" int hs_rf_spectrum(int nlay, const double *h, const double *vp, const double *vs, const double *rho, double p,
                              double gauss, int nsamp, double fsamp, double tshift, double nsv, int waveno, int nout,
                              double *spec)
{
    RfLaunch P;
    std::memset(&P, 0, sizeof(P));
    rf_fill_launch(P, p, gauss, nsamp, fsamp, tshift, nsv, waveno, nout);
    P.sigma = std::nan("");
    P.Lmax = nlay;
    const RfLayout lo = rf_layout(nlay, nsamp);
    std::vector<double> S(lo.per_model, 0.0), ftab((size_t)RF_FTAB * P.nfreq);
    rf_fill_freq_table(P, ftab.data());
    for (int i = 0; i < nlay; i++) rf_phase1_layer(S.data(), lo, nlay, i, h, vp, vs, rho, nullptr, nullptr, 0);
    for (int i = 0; i < nlay; i++) rf_phase2_interface(S.data(), lo, P, nlay, i, vp[0], vs[0]);
    for (int j = 0; j < P.nfreq; j++) {
        const cd v = j < P.nact ? rf_phase3_task(S.data(), lo, P, nlay, j, rf_freq_load(ftab.data(), j)) : mk(0., 0.);
        spec[2 * j] = v.re; spec[2 * j + 1] = v.im;
    }
    return P.nact;
}
