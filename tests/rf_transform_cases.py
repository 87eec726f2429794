"""Shared by test_rf_transform.py (CPU tier) and test_gpu_rf_transform.py (GPU tier): the host twin of
bh_selftest_rf_transform (tests/hostsim/rf_transform_sim.cpp, the flags of conftest's hostsim_devmath build), the device
call, the spectra, the extended-precision reference of the inverse transform and the bound both tiers assert.
The twin is given the twiddle table of the library's own host build (bh_rf_twiddles), the one the device reads.

The reference restates greens.cpp:136-158 (iftr), :161-194 (iftr2) and fork.cpp:10-60 (ccfork, signi = +1), not the
kernel: entries 0 .. n/2 as given, entries above the conjugate mirror cx[i] = conj(cx[n - i]) -- the imaginary parts of
the DC and the Nyquist bin are kept, as the reference keeps them --,

    y[k] = (1/n) sum_j x[j] exp(+2 pi i j k / n)        (ccfork scales by sqrt(1/n), iftr by 1/sqrt(n))

and f = Re y (iftr) or, for x = x1 + i x2, f1 = Re y, f2 = Im y (iftr2).  In iftr the imaginary parts of x[0] and x[n/2]
contribute i (Im x[0] + (-1)^k Im x[n/2]) / n to y[k] and so nothing to f; in iftr2 those of x2 enter f1 negated and
those of x1 enter f2.  numpy.longdouble is the x87 format here (64 significant bits, 2^-11 of a double's unit roundoff).
A direct O(n^2) sum for n <= 512, and for every n a plain radix-2 decimation-in-time FFT in long double that
test_rf_transform.py checks against the direct sum where both exist.

THE BOUND (derived, not measured).  Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 24.2: the
Cooley-Tukey radix-2 transform y^ of x with t = log2 n stages and twiddles of absolute error <= mu obeys

    ||y^ - y||_2 / ||y||_2 <= t eta / (1 - t eta),    eta = mu + gamma_4 (sqrt 2 + mu),    gamma_4 = 4u / (1 - 4u),

u = 2^-53.  The radix-4 passes form the products and sums of the radix-2 stages in their order (rf_core.h).  Phase 4's
sums are compiled without contraction; the complex product w b is bh_common.h's operator*, which the device compiles
contracted into fma(w.re, b.re, -(w.im b.im)), fma(w.im, b.re, w.re b.im) and the twin is built to form the same way
(BH_HOSTSIM_FUSED_CMUL): one rounding fewer per component than the product the theorem assumes, so its model of
arithmetic (a complex product within sqrt 2 gamma_2, a sum within gamma_1) holds with room.  Twiddles (rf_host.h,
rf_fill_twiddles, as fork.cpp:50-51): exp(i fl(fl(M_PI m) / l)).  M_PI is pi (1 + 0.35u'), |u'| <= u; the product
rounds once, the quotient once, so the angle, below pi, carries at most (0.35 + 2) u pi < 7.4u; glibc's sine and cosine
at under 1 ulp (2u relative at worst, of values <= 1) add 2 sqrt 2 u: mu <= 10.3u, eta <= 10.3u + 4u (1.4143) + O(u^2)
<= 16u.  The two scalings (sc = fl(sqrt(fl(1/n))), at most u/2 off; qn = fl(1 / fl(sqrt n)), at most u off; one
rounding for each of the two products) add 3.5u <= 4u.  Hence

    ||f^ - f||_2 <= (16 log2 n + 4) u ||y||_2,

y the complex transform, and every component's absolute error obeys the same figure (|e_k| <= ||e||_2).

Rechecked: one slip, and why the figure stands.  The paired form first rounds x1 + i x2 (rf_fft_pair_entry: one addition
per component), an input perturbation of at most u ||x||_2, which the derivation above does not count and which adds u
||y||_2 (the transform is unitary up to its scale) -- 4.5u for the term that is given as 4u.  But l is a power of two, so
the quotient fl(M_PI m) / l is exact and the angle carries (0.35 + 1) u pi < 4.3u: mu <= 7.1u (test_twiddle_table
measures it and asserts the 10.3u above), eta <= 12.8u, and (16 log2 n + 4) u exceeds the corrected (12.8 log2 n + 4.5) u
at every n >= 2.  Both forms are therefore held to (16 log2 n + 4) u ||y||_2 as first derived."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
LENGTHS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
MU_BOUND = 10.3          # twiddle error in units of u (the derivation above)
DIRECT_MAX = 512         # the direct O(n^2) sum up to here
LDS_LIMIT = 160 * 1024   # what the library's own launches allow a workgroup (host_common.h: kLdsLimit)
_SIM = {}


def bound_u(n):
    """the bound in units of u ||y||_2"""
    return 16.0 * int(np.log2(n)) + 4.0


def transform_sim():
    """g++ build of rf_transform_sim.cpp with the device math of bh_math.h"""
    if 'hs' in _SIM:
        return _SIM['hs']
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so, src = os.path.join(d, 'librf_transform_sim.so'), os.path.join(d, 'rf_transform_sim.cpp')
    deps = [src] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', f) for f in ('bh_common.h', 'bh_math.h', 'rf_core.h', 'rf_host.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        fma = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + fma + ['-o', so, src], check=True)
    hs = C.CDLL(so)
    hs.hs_rf_transform.restype = C.c_int
    hs.hs_rf_transform.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    hs.hs_rf_twiddles.restype = None
    hs.hs_rf_twiddles.argtypes = [C.c_int, C.c_void_p]
    hs.hs_rf_per_model.restype = C.c_int
    hs.hs_rf_per_model.argtypes = [C.c_int, C.c_int]
    _SIM['hs'] = hs
    return hs


# ---- spectra ---------------------------------------------------------------------------------------------------------
def spectra(n):
    """[(name, complex128 [n/2 + 1])]: unit impulses 1, i, 1 + i at bins 0, 1, 2, n/4, n/2 - 1, n/2 (each bin once where
    two coincide), all ones, alternating signs, full-band complex normal (DC and Nyquist complex too) and a
    Gauss-filtered normal spectrum that falls to 1e-24 at 3n/8 and is exactly zero from there up."""
    nf = n // 2 + 1
    out = []
    for b in sorted({0, 1, 2, n // 4, n // 2 - 1, n // 2}):
        for tag, v in (('1', 1.0), ('i', 1.0j), ('1+i', 1.0 + 1.0j)):
            x = np.zeros(nf, dtype=np.complex128)
            x[b] = v
            out.append(('impulse %s at %d' % (tag, b), x))
    out.append(('ones', np.ones(nf, dtype=np.complex128)))
    out.append(('alternating', ((-1.0) ** np.arange(nf)).astype(np.complex128)))
    rs = np.random.RandomState(1000 + n)
    out.append(('normal', rs.standard_normal(nf) + 1j * rs.standard_normal(nf)))
    jc = 3 * n // 8
    g = (rs.standard_normal(nf) + 1j * rs.standard_normal(nf)) * np.exp(np.log(1e-24) * (np.arange(nf) / float(jc)) ** 2)
    g[jc:] = 0.0
    out.append(('gauss', g))
    return out


def pairs(n):
    """[(name, x1, x2)]: every spectrum once as the first and once as the second channel"""
    s = spectra(n)
    return [('%s | %s' % (s[k][0], s[(k + 7) % len(s)][0]), s[k][1], s[(k + 7) % len(s)][1]) for k in range(len(s))]


def as_doubles(x):
    """complex [.., nf] -> float64 [.., nf, 2]"""
    x = np.asarray(x, dtype=np.complex128)
    return np.ascontiguousarray(np.stack((x.real, x.imag), axis=-1))


# ---- the two builds -----------------------------------------------------------------------------------------------------
def library_table(n):
    """The twiddle table as the library's own host code builds it (bh_rf_twiddles: what get_twiddles of rf_capi.hip uploads), [2n].  The
    twin takes this table: rf_fill_twiddles compiled by g++ into the twin differs from the library's build of it in the
    last bit of one entry (n = 4096: the sine of pi 1955 / 2048) -- glibc's values both, through different calls."""
    if ('T', n) not in _SIM:
        import bayhunter_amd
        from bayhunter_amd import _lib
        bayhunter_amd.build()
        tw = np.zeros(2 * n)
        _lib.check(bayhunter_amd.load().bh_rf_twiddles(n, tw.ctypes.data))
        _SIM[('T', n)] = tw
    return _SIM[('T', n)]


def host(n, spec, nout=None, Lmax=10, radix4=True):
    """one buffer through the host twin, with the library's twiddle table.  spec complex [nf] (single) or [2][nf]
    (paired); [nout] or [2][nout]"""
    spec = np.asarray(spec)
    paired = spec.ndim == 2
    nout = n if nout is None else nout
    a = as_doubles(spec)
    out = np.full((2 if paired else 1, nout), 7.0)
    assert transform_sim().hs_rf_transform(n, Lmax, 1 if paired else 0, a.ctypes.data, nout, out.ctypes.data,
                                           1 if radix4 else 0, library_table(n).ctypes.data) == 0
    return out if paired else out[0]


def lds_bytes(n, Lmax, M, paired):
    """rf_lds_bytes (kernels.hip) of M buffers"""
    return 8 * M * (transform_sim().hs_rf_per_model(Lmax, n) + (4 * (n // 2 + 1) if paired else 0))


def device_rc(lib, n, Lmax, M, specs, nout, paired):
    """bh_selftest_rf_transform on specs complex [B][nf] or [B][2][nf]: (return code, out [B][nch][nout])"""
    a = as_doubles(specs)
    B = a.shape[0]
    out = np.full((B, 2 if paired else 1, nout), 7.0)
    rc = lib.bh_selftest_rf_transform(n, Lmax, M, B, 1 if paired else 0, a.ctypes.data, nout, out.ctypes.data)
    return rc, out


def same_bits(a, b):
    """equal as int64 views wherever neither is NaN, and NaN in the same places"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


# ---- extended precision ---------------------------------------------------------------------------------------------------
PI_LD = LD(4) * np.arctan(LD(1))
_W = {}


def roots(n):
    """exp(+2 pi i m / n), m < n, in long double"""
    if n not in _W:
        ang = (LD(2) * PI_LD) * np.arange(n).astype(LD) / LD(n)
        _W[n] = (np.cos(ang) + CLD(1j) * np.sin(ang)).astype(CLD)
    return _W[n]


def mirror(x):
    """greens.cpp:149-152: [.., n/2 + 1] -> [.., n], cx[i] = conj(cx[n - i]) above n/2"""
    x = np.asarray(x).astype(CLD)
    return np.concatenate((x, np.conj(x[..., -2:0:-1])), axis=-1)


def _fft_ld(x, w):
    n = x.shape[-1]
    if n == 1:
        return x
    e, o = _fft_ld(x[..., ::2], w[::2]), _fft_ld(x[..., 1::2], w[::2])
    t = w[:n // 2] * o
    return np.concatenate((e + t, e - t), axis=-1)


def inverse_fft(x):
    """y[k] = (1/n) sum_j x[j] exp(+2 pi i j k / n) of the full complex [.., n] by radix-2 decimation in time"""
    n = x.shape[-1]
    return _fft_ld(x.astype(CLD), roots(n)) / LD(n)


def inverse_direct(x):
    """the same by the direct sum"""
    n = x.shape[-1]
    assert n <= DIRECT_MAX
    if ('D', n) not in _W:
        j = np.arange(n)
        _W[('D', n)] = roots(n)[np.outer(j, j) % n]
    return (x.astype(CLD) @ _W[('D', n)]) / LD(n)


def reference(spec, direct=False):
    """The complex y of a half spectrum [nf] (iftr: the result is its real part) or of a pair [2][nf] (iftr2: x1 + i x2,
    the results are its real and imaginary part), in long double."""
    spec = np.asarray(spec)
    x = mirror(spec)
    if spec.ndim == 2:
        x = x[0] + CLD(1j) * x[1]
    return inverse_direct(x) if direct else inverse_fft(x)


def error_in_u(got, y):
    """||got - f||_2 / (u ||y||_2) for got [n] against Re y, or got [2][n] against (Re y, Im y)"""
    got = np.asarray(got, dtype=np.float64)
    if got.ndim == 2:
        e = np.concatenate((got[0].astype(LD) - y.real, got[1].astype(LD) - y.imag))
    else:
        e = got.astype(LD) - y.real
    norm = np.sqrt(np.sum(np.abs(y) ** 2))
    assert norm > 0
    return float(np.sqrt(np.sum(e * e)) / (LD(U) * norm))
