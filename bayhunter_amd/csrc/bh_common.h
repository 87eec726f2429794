// bh_common.h -- shared definitions for the HIP kernels of libbayhunter_amd.
//
// The per-lane solver cores (swd_core.h, rf_core.h) are plain C++ functions marked BH_DEV.  hipcc
// compiles them for gfx950; tests/hostsim/ compiles the very same headers with g++ (BH_HOSTSIM) to
// check the control-flow transformation against the oracle bit for bit on the CPU.  The host build
// is test infrastructure only: nothing in the shipped library or Python package uses it.
#pragma once

#if defined(BH_HOSTSIM)
#include <cmath>
#define BH_DEV static inline
#define BH_HD static inline
#define BH_RESTRICT __restrict__
#else
#include <hip/hip_runtime.h>
#define BH_DEV __device__ __forceinline__
#define BH_HD __host__ __device__ __forceinline__
#define BH_RESTRICT __restrict__
#endif

namespace bh {

#if defined(BH_HOSTSIM)
using std::copysign;
using std::cos;
using std::exp;
using std::fabs;
using std::log;
using std::sin;
using std::sqrt;
#else
#endif

// ---- IEEE division, shared-divisor form ------------------------------------------------------------
// hipcc expands `a / b` (fp64) to v_div_scale x2, v_rcp, two Newton steps on the reciprocal, q0 = a*r,
// rem = fma(-b, q0, a), v_div_fmas, v_div_fixup.  The scale / fix-up instructions only act on
// denormal, overflowing or non-finite operands; for the normal-range operands of the period
// equation the quotient is exactly q1 = fma(rem, r, q0).  Recip keeps the refined reciprocal so that
// the quotients by one divisor (three by rho, five by the normalisation factor of normc) share it:
// 5 instructions per reciprocal (one of them v_rcp_f64) + 3 per quotient instead of 11 per quotient
// (divisors that are a root or an exact square get their reciprocal cheaper still, below).  Bit-identical to `/` there
// (bh_selftest / tests/test_gpu_parity.py::test_division_selftest); a zero numerator yields +0 where
// IEEE gives -0 for -0/b, non-finite operands may yield NaN where IEEE gives Inf/0.
// The host replay uses the plain operator.
#if defined(BH_HOSTSIM)
struct Recip { double b; };
BH_DEV Recip recip_of(double b) { Recip R; R.b = b; return R; }
BH_DEV double qdiv(double a, const Recip &R) { return a / R.b; }
#else
struct Recip { double b, r; };
BH_DEV Recip recip_of(double b)
{
    Recip R;
    R.b = b;
    double r = __builtin_amdgcn_rcp(b);
    r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
    R.r = r;
    return R;
}
BH_DEV double qdiv(double a, const Recip &R)
{
    const double q0 = a * R.r;
    return __builtin_fma(__builtin_fma(-R.b, q0, a), R.r, q0);
}
#endif
BH_DEV double xdiv(double a, double b) { return qdiv(a, recip_of(b)); }

// IEEE square root for arguments that are zero or in the normal range (no denormals, no Inf): the
// compiler's own sequence (v_rsq, one coupled Newton step, two residual corrections) without its
// 2^256 range scaling.  Bit-identical to sqrt() there (bh_selftest_division).
//
// The coupled step carries h ~ 1/(2 sqrt(x)) next to g ~ sqrt(x), so a quotient by the root needs no
// v_rcp_f64 of its own: xsqrt_recip_nz returns Recip{g, r} with r = 2h after STEPS Newton corrections
// against the rounded root g (2 fma each).  With r = (1/b)(1 + d), qdiv's result before its final rounding
// is (a/b)(1 - d^2) whatever q0's rounding was: a quotient moves only when a/b lies within d^2 of a rounding
// boundary, about 2 d^2 / 2^-53 of all quotients.  Measured on 2^26 + 2^24 random operands (exponents
// +-40 / +-300; two quotients each) against `/` and sqrt(), with the largest |1 - b r|:
//     STEPS  mismatches  max |1 - b r|     expected mismatches per quotient
//     0      0           38.3 x 2^-53      ~3e-13: none in the sample, one per ~10^3 steps of the headline
//                                          workload (3e9 such quotients a step).  Not shipped.
//     1      0            1.00 x 2^-53     that of recip_of itself (1.00 x 2^-53 in the same run).  Shipped.
//     2      0            1.00 x 2^-53     no better than 1
// _nz: no select for x == 0 (g and r are NaN there).  For the layer steps of the period equations: a
// root vanishes only when wvno equals the layer's wavenumber, and that branch reads neither the root
// nor its product with the thickness (swd_var, swd_love_layer; tests/test_gpu_recip_reuse.py).
// recip_sq: the Recip of b*b from the Recip of b, for a b whose square is exact (an fp32 value widened
// to fp64): the product of the reciprocals (|1 - b r| up to 2.99 x 2^-53, 0 mismatches in the sample) and
// one correction for the same reason as above.
// Per quotient by a root 3 + 3 instructions, by the square 3 + 3, instead of 5 + 3 with a v_rcp_f64 each.
#if defined(BH_HOSTSIM)
BH_DEV double xsqrt(double x) { return sqrt(x); }
BH_DEV Recip xsqrt_recip_nz(double x) { return recip_of(sqrt(x)); }
BH_DEV Recip recip_sq(const Recip &R) { return recip_of(R.b * R.b); }
#else
BH_DEV void xsqrt_gh(double x, double &g, double &h)
{
    const double y = __builtin_amdgcn_rsq(x);
    g = x * y; h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
    g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
}
BH_DEV double xsqrt(double x)
{
    double g, h;
    xsqrt_gh(x, g, h);
    return (x == 0.0) ? x : g;
}
enum { BH_ROOT_RECIP_STEPS = 1 };
template <int STEPS>
BH_DEV Recip xsqrt_recip_nz_steps(double x)
{
    Recip R;
    double h;
    xsqrt_gh(x, R.b, h);
    double r = h + h;
    for (int i = 0; i < STEPS; i++) r = __builtin_fma(r, __builtin_fma(-R.b, r, 1.0), r);
    R.r = r;
    return R;
}
BH_DEV Recip xsqrt_recip_nz(double x) { return xsqrt_recip_nz_steps<BH_ROOT_RECIP_STEPS>(x); }
BH_DEV Recip recip_sq(const Recip &R)
{
    Recip S;
    S.b = R.b * R.b;
    const double r = R.r * R.r;
    S.r = __builtin_fma(r, __builtin_fma(-S.b, r, 1.0), r);
    return S;
}
#endif

// bh_fma_exact2(a, k, c) = fma(a, k, c) for k = +-2^n: the bits of the unfused `a * k + c`, and of `(a + c / k) * k`, in
// one instruction instead of two.  A product with a power of two is exact unless it over- or underflows, so either unfused
// form rounds once -- the sum -- and rounding commutes with the scaling: round(a + c / k) k = round(a k + c), which
// is what the fused form returns.  Where a is itself a rounded product, round(x y) k = round(x y k) for the same
// reason: an exact factor may be taken out of a product and handed to the fused form.  The fused form never rounds
// a * k, so the one condition is that the UNFUSED form did not either: at each use the caller states why the scaled
// term (and, for a factor taken out of a product, the product) is zero or normal and far from overflow.  The library
// is compiled with -ffp-contract=off: nothing is fused that is not written as a fusion.
BH_DEV double bh_fma_exact2(double a, double k, double c) { return __builtin_fma(a, k, c); }

BH_DEV double dsign1(double x) { return copysign(1.0, x); }
// dsign(1, a) != dsign(1, b), equivalently dsign(1, a) * dsign(1, b) < 0 (the reference's sign tests,
// surfdisp96.f:431,461,600,616): the sign bits differ.  One xor instead of two copysigns and a product;
// the same truth value for every pair of operands, zeros and NaNs included.
#if defined(BH_HOSTSIM)
BH_DEV bool bh_signs_differ(double a, double b) { return std::signbit(a) != std::signbit(b); }
#else
BH_DEV bool bh_signs_differ(double a, double b) { return (__double2hiint(a) ^ __double2hiint(b)) < 0; }
#endif
BH_DEV double bh_fmax(double a, double b) { return __builtin_fmax(a, b); }
BH_DEV double dmin(double a, double b) { return a < b ? a : b; }
BH_DEV double dmax(double a, double b) { return a > b ? a : b; }

// ---- complex fp64 --------------------------------------------------------------------------
// Complex arithmetic is only used by the receiver-function path, which is tolerance-checked
// (|diff| <= 1e-10, observed 1e-13): it may use FMA contraction.  The surface-wave path (real
// arithmetic, exact replay) is compiled with contraction off.
#if !defined(BH_HOSTSIM)
#pragma clang fp contract(fast)
#endif
struct cd {
    double re, im;
};
BH_DEV cd mk(double re, double im) { cd r; r.re = re; r.im = im; return r; }
BH_DEV cd operator+(cd a, cd b) { return mk(a.re + b.re, a.im + b.im); }
BH_DEV cd operator-(cd a, cd b) { return mk(a.re - b.re, a.im - b.im); }
BH_DEV cd operator-(cd a) { return mk(-a.re, -a.im); }
#if defined(BH_HOSTSIM) && defined(BH_HOSTSIM_FUSED_CMUL)
// The device compiles this operator under contract(fast) above, and the flag goes with the operator's instructions into
// every caller -- phase 4's butterflies included, whose own sums stay separate additions (rf_core.h).  What the compiler
// makes of the two halves there (the listing of rf_block_fft: v_mul, v_mul, v_fma, v_fmac per product) is
// fma(a.re, b.re, -(a.im b.im)) and fma(a.im, b.re, a.re b.im) -- the real part as cmul (below) writes it, the imaginary
// part with the other product rounded.  A host build that is to return the device's bits for a sequence of such products
// (tests/hostsim/rf_transform_sim.cpp) asks for that form; tests/test_gpu_rf_transform.py is what holds it to the device.
BH_DEV cd operator*(cd a, cd b)
{
    return mk(__builtin_fma(a.re, b.re, -(a.im * b.im)), __builtin_fma(a.im, b.re, a.re * b.im));
}
#else
BH_DEV cd operator*(cd a, cd b) { return mk(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
#endif
BH_DEV cd operator*(cd a, double r) { return mk(a.re * r, a.im * r); }
BH_DEV cd operator*(double r, cd a) { return mk(a.re * r, a.im * r); }
BH_DEV cd operator/(cd a, double r) { return mk(a.re / r, a.im / r); }
BH_DEV cd operator+(double r, cd a) { return mk(a.re + r, a.im); }
BH_DEV cd operator+(cd a, double r) { return mk(a.re + r, a.im); }
BH_DEV cd operator-(cd a, double r) { return mk(a.re - r, a.im); }
BH_DEV cd conj(cd a) { return mk(a.re, -a.im); }

// complex / complex: Smith's algorithm as in libgcc's __divdc3 (the reference's std::complex
// division lowers to it); the NaN/Inf recovery tail of __divdc3 is not needed here.
// Not contracted: only the set-up phase of the receiver function divides complex by complex (rf_coeffs, rf_coeffm,
// rf_displacement2: once per interface), and that phase follows the reference expression by expression.  Smith's
// numerators a (c/d) + b cancel, so a fused product there moved a component by up to 272 ulp from libgcc's quotient
// (4 ulp of the modulus; tests/test_gpu_math_probe.py); with every product rounded the device's quotient is libgcc's.
#if !defined(BH_HOSTSIM)
#pragma clang fp contract(off)
#endif
BH_DEV cd operator/(cd x, cd y)
{
    double a = x.re, b = x.im, c = y.re, d = y.im, ratio, denom;
    if (fabs(c) < fabs(d)) {
        ratio = c / d;
        denom = (c * ratio) + d;
        return mk(((a * ratio) + b) / denom, ((b * ratio) - a) / denom);
    }
    ratio = d / c;
    denom = (d * ratio) + c;
    return mk(((b * ratio) + a) / denom, (b - (a * ratio)) / denom);
}
BH_DEV cd rdiv(double x, cd y) { return mk(x, 0.0) / y; }
#if !defined(BH_HOSTSIM)
#pragma clang fp contract(fast)
#endif
// Fast reciprocal / square root for the tolerance-checked receiver-function recursion: hardware
// seed (v_rcp_f64 / v_rsq_f64) + Newton steps, half the instructions of the IEEE sequences.  Measured on the device
// against long double, 2^19 operands each of magnitude 2^-20 .. 2^20 and 2^-300 .. 2^300 (bh_selftest_math,
// tests/test_gpu_math_probe.py): frcp, fsqrt and the root of fsqrt_hinv 0.500 ulp at worst, i.e. no operand found on
// which they are not correctly rounded; h of fsqrt_hinv 1.49 ulp (what 0.5 / sqrt(x) in two roundings gives: 1.49);
// crecip 2.72 ulp per component, csqrt_fast 2.64.
// Arguments there are well scaled (1e-6..1e6) and non-zero: fsqrt has no select for a zero or negative
// argument (it is only asked for |z| of a slowness, which cannot vanish; a NaN stays a NaN).
#if defined(BH_HOSTSIM)
BH_DEV double frcp(double x) { return 1.0 / x; }
BH_DEV double fsqrt(double x) { return sqrt(x); }
#else
BH_DEV double frcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}
BH_DEV double fsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);          // ~ 1/sqrt(x)
    double g = x * y, h = 0.5 * y;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    return __builtin_fma(__builtin_fma(-g, g, x), h, g);
}
#endif

// Products of the receiver-function recursion as explicit multiply-add chains.  Left to contraction, a sum
// of two complex products becomes two contracted halves and a separate add (five instructions per
// component instead of four); written out, a product is 2 mul + 2 fma and every further term 4 fma.  The
// first factor may be real (the interface coefficients of a stack without post-critical waves).
BH_DEV cd cmul(cd a, cd b)
{
    return mk(__builtin_fma(a.re, b.re, -(a.im * b.im)), __builtin_fma(a.re, b.im, a.im * b.re));
}
BH_DEV cd cmul(double a, cd b) { return mk(a * b.re, a * b.im); }
BH_DEV cd cmadd(cd acc, cd a, cd b)               // acc + a*b
{
    return mk(__builtin_fma(a.re, b.re, __builtin_fma(-a.im, b.im, acc.re)),
              __builtin_fma(a.re, b.im, __builtin_fma(a.im, b.re, acc.im)));
}
BH_DEV cd cmadd(cd acc, double a, cd b) { return mk(__builtin_fma(a, b.re, acc.re), __builtin_fma(a, b.im, acc.im)); }
BH_DEV cd cmsub(cd acc, cd a, cd b)               // acc - a*b
{
    return mk(__builtin_fma(-a.re, b.re, __builtin_fma(a.im, b.im, acc.re)),
              __builtin_fma(-a.re, b.im, __builtin_fma(-a.im, b.re, acc.im)));
}
BH_DEV cd cmsub(cd acc, double a, cd b) { return mk(__builtin_fma(-a, b.re, acc.re), __builtin_fma(-a, b.im, acc.im)); }
BH_DEV cd cmadd(double acc, cd a, cd b) { return cmadd(mk(acc, 0.0), a, b); }
BH_DEV cd cmadd(double acc, double a, cd b) { return mk(__builtin_fma(a, b.re, acc), a * b.im); }

// 1/z = conj(z)/|z|^2: one real reciprocal instead of Smith's three divisions
BH_DEV cd crecip(cd z)
{
    double r = frcp(z.re * z.re + z.im * z.im);
    return mk(z.re * r, -(z.im * r));
}

// sqrt(x) and 1/(2 sqrt(x)) from one v_rsq_f64 seed (the coupled Newton iteration of fsqrt carries both)
#if defined(BH_HOSTSIM)
BH_DEV void fsqrt_hinv(double x, double *g, double *h) { *g = sqrt(x); *h = 0.5 / *g; }
#else
BH_DEV void fsqrt_hinv(double x, double *gout, double *hout)
{
    double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    // One more step on h, against the refined g.  r = 1/2 - h g is half of Newton's residual 1 - 2 h g, so the step is
    // h + h (2 r).  (It was h + h r until the device test of this function: that halves the error where Newton
    // squares it -- 10.0 ulp at worst in h, 18.7 in csqrt_fast's smaller component.  The coupled step above is a
    // different iteration: there g and h carry the same error and r corrects both.)
    r = __builtin_fma(-h, g, 0.5);
    h = __builtin_fma(h, r + r, h);
    *gout = g;
    *hout = h;
}
#endif

// principal square root for generic complex arguments of the recursion (im != 0): with m = the larger of
// the two roots sqrt((|z| +- re)/2), the other one is im / (2 m)
BH_DEV cd csqrt_fast(cd z)
{
    double re = z.re, im = z.im;
    double d = fsqrt(re * re + im * im), m, hinv;
    fsqrt_hinv(0.5 * (d + fabs(re)), &m, &hinv);
    const double o = im * hinv;                   // im / (2 m)
    return (re > 0) ? mk(m, o) : mk(fabs(o), copysign(m, im));
}

// principal square root, glibc csqrt's formulation for finite non-zero arguments, except that |z| is sqrt(re^2 + im^2)
// where glibc takes hypot(re, im): bit-equal to glibc for im == 0 (all the library asks: the vertical slownesses of
// rf_coeffm) and for re == 0, up to 2 ulp from it for 6 % of generic arguments (tests/test_math_probe.py)
BH_DEV cd csqrt_(cd z)
{
    double re = z.re, im = z.im;
    if (im == 0.0) {
        if (re < 0.0) return mk(0.0, copysign(sqrt(-re), im));
        return mk(fabs(sqrt(re)), copysign(0.0, im));
    }
    if (re == 0.0) {
        double r = sqrt(0.5 * fabs(im));
        return mk(r, copysign(r, im));
    }
    double d = sqrt(re * re + im * im), r, s;
    if (re > 0) {
        r = sqrt(0.5 * (d + re));
        s = 0.5 * (im / r);
    } else {
        s = sqrt(0.5 * (d - re));
        r = fabs(0.5 * (im / s));
    }
    return mk(r, copysign(s, im));
}


// ---- complex 2x2 (rfmini cmat2.h) ------------------------------------------------------------
struct cm2 {
    cd c11, c12, c21, c22;
};
BH_DEV cm2 operator*(const cm2 &x, const cm2 &y)
{
    cm2 r;
    r.c11 = x.c11 * y.c11 + x.c12 * y.c21;
    r.c12 = x.c11 * y.c12 + x.c12 * y.c22;
    r.c21 = x.c21 * y.c11 + x.c22 * y.c21;
    r.c22 = x.c21 * y.c12 + x.c22 * y.c22;
    return r;
}
BH_DEV cm2 operator+(const cm2 &x, const cm2 &y)
{
    cm2 r;
    r.c11 = x.c11 + y.c11; r.c12 = x.c12 + y.c12; r.c21 = x.c21 + y.c21; r.c22 = x.c22 + y.c22;
    return r;
}

// real 2x2: the interface coefficient matrices of a model are real when no wave is post-critical anywhere
// in the stack (the teleseismic case), and a complex product with a zero imaginary part is the real one
// (cmul / cmadd / cmsub with a real first factor)
struct rm2 {
    double c11, c12, c21, c22;
};

#if !defined(BH_HOSTSIM)
#pragma clang fp contract(off)
#endif

}  // namespace bh
