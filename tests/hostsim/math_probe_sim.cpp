// TEST INFRASTRUCTURE ONLY: the op table of bayhunter_amd/csrc/math_probe.h compiled by g++ -- the host side of every
// #if defined(BH_HOSTSIM) of the primitives, with the device math of bh_math.h (the flags of conftest's hostsim_devmath
// build; tests/math_probe_cases.py builds it).  One element at a time: what the kernel of math_probe.hip computes per
// thread, and rf_cexp_pair's wave-uniform choice taken per element.
#define BH_HOSTSIM 1
#include <cmath>
#include <cstring>
#include "../../bayhunter_amd/csrc/math_probe.h"

// in [n][MP_IN], out [n][MP_OUT]; 1 for an unknown op or n < 0 (as bh_selftest_math refuses them)
extern "C" int hs_math_probe(int op, long n, const double *in, double *out)
{
    if (op < 0 || op >= bh::MP_NOPS || n < 0 || !in || !out) return 1;
    for (long i = 0; i < n; i++) bh::math_probe_apply(op, in + bh::MP_IN * i, out + bh::MP_OUT * i);
    return 0;
}

extern "C" int hs_math_probe_nops(void) { return bh::MP_NOPS; }
extern "C" double hs_math_probe_exp_small_bound(void) { return RF_EXP_SMALL; }

// What the comments of bh_common.h name as the formulations of operator/(cd, cd) and csqrt_: g++'s std::complex<double>
// quotient (libgcc's __divdc3) for what = 0, std::sqrt (glibc's csqrt) for what = 1.  in [n][4], out [n][2].
#include <complex>
extern "C" void hs_std_complex(int what, long n, const double *in, double *out)
{
    for (long i = 0; i < n; i++) {
        const std::complex<double> x(in[4 * i], in[4 * i + 1]), y(in[4 * i + 2], in[4 * i + 3]);
        const std::complex<double> r = what == 0 ? x / y : std::sqrt(x);
        out[2 * i] = r.real(); out[2 * i + 1] = r.imag();
    }
}
