// TEST INFRASTRUCTURE ONLY: the host twin of bh_selftest_rf_transform (csrc/rf_probe.hip) -- phase 4 of rf_kernel on one
// buffer laid out like a model's LDS block, step by step as the probe's workgroup runs it, with the functions the device
// runs (rf_core.h: rf_xst, rf_fft_hermitian, rf_fft_pair_entry, the butterflies and the plan through rf_host.h's
// rf_host_fft) and the table of rf_fill_twiddles.  Phase 4's own sums and scalings are compiled without contraction on
// both sides; the complex product of the butterflies is bh_common.h's operator*, which the device compiles contracted:
// BH_HOSTSIM_FUSED_CMUL gives this build the same two fused multiply-adds, so that every operation here is the
// device's.  Built by tests/rf_transform_cases.py with the flags of the device-math replay (conftest's
// hostsim_devmath build; -mfma there makes the fma one instruction, its value is the correctly rounded one either way).
#define BH_HOSTSIM 1
#define BH_HOSTSIM_FUSED_CMUL 1
#include <cmath>
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/rf_host.h"

using namespace bh;

// spec [paired ? 2 : 1][nsamp / 2 + 1][2], out [paired ? 2 : 1][nout].  radix4 = 0: every stage as a radix-2 stage.
// 1 for the arguments bh_selftest_rf_transform refuses (but for the LDS rule, which is the library's).
// table: the 2 nsamp twiddle doubles to use (the library's own, bh_rf_twiddles), or null for this build's rf_fill_twiddles.
extern "C" int hs_rf_transform(int nsamp, int Lmax, int paired, const double *spec, int nout, double *out, int radix4,
                               const double *table)
{
    if (nsamp < 8 || nsamp > 4096 || (nsamp & (nsamp - 1)) || Lmax < 1 || Lmax > 100 || nout < 1 || nout > nsamp ||
        !spec || !out)
        return 1;
    RfLaunch P = RfLaunch();
    rf_fill_launch(P, 0.0, 1.0, nsamp, 1.0, 0.0, -1.0, 0, nout);
    P.Lmax = Lmax;
    const RfLayout lo = rf_layout(Lmax, nsamp);
    const int n = nsamp, nf = P.nfreq;
    std::vector<double> buf((size_t)lo.per_model + (paired ? 4 * nf : 0), std::nan("")), tw(2 * (size_t)n);
    double *S = buf.data();
    if (table) std::memcpy(tw.data(), table, tw.size() * sizeof(double));
    else rf_fill_twiddles(tw.data(), n);
    for (int j = 0; j < nf; j++) {
        rf_xst(S, j, ld_cd(spec + 2 * j));
        if (paired) {
            st_cd(S + lo.per_model + 2 * j, ld_cd(spec + 2 * j));
            st_cd(S + lo.per_model + 2 * nf + 2 * j, ld_cd(spec + 2 * nf + 2 * j));
        }
    }
    for (int i = n / 2 + 1; i < n; i++) rf_fft_hermitian(S, n, i);
    rf_host_fft(S, tw.data(), P, radix4 != 0);
    for (int i = 0; i < nout; i++) out[i] = P.qn * S[2 * rf_swz(i)];
    if (paired) {
        for (int i = 0; i < n; i++) rf_xst(S, i, rf_fft_pair_entry(S + lo.per_model, S + lo.per_model + 2 * nf, n, i));
        rf_host_fft(S, tw.data(), P, radix4 != 0);
        for (int i = 0; i < nout; i++) {
            out[i] = P.qn * S[2 * rf_swz(i)];
            out[nout + i] = P.qn * S[2 * rf_swz(i) + 1];
        }
    }
    return 0;
}

// the table of rf_fill_twiddles, [2 nsamp]
extern "C" void hs_rf_twiddles(int nsamp, double *tw) { rf_fill_twiddles(tw, nsamp); }

// the pitch of a model's block in doubles
extern "C" int hs_rf_per_model(int Lmax, int nsamp) { return rf_layout(Lmax, nsamp).per_model; }
