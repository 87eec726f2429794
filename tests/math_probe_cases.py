"""Shared by test_math_probe.py (CPU tier) and test_gpu_math_probe.py (GPU tier): the host build of the op table of
bayhunter_amd/csrc/math_probe.h (tests/hostsim/math_probe_sim.cpp, the flags of conftest's hostsim_devmath build), the
device call (bh_selftest_math), the input sets -- every one from a fixed seed -- and the extended-precision references.

numpy.longdouble is the x87 format here: 64 significant bits, 2^-11 ulp of a double, and glibc's sinl / cosl / expl
reduce their arguments exactly (tests/test_hostsim.py::test_math_accuracy relies on the same)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
MP_IN, MP_OUT = 6, 4
# enum MathProbeOp, math_probe.h
OP_NAMES = ['SINCOS', 'EXP', 'EXP_BOUNDED', 'EXP_SMALL', 'CEXP', 'CEXP_BOUNDED', 'CEXP_PAIR', 'FRCP', 'FSQRT', 'FSQRT_HINV',
            'CRECIP', 'CSQRT_FAST', 'CSQRT', 'CDIV', 'CMUL', 'CMADD', 'CMSUB', 'NEGATE_IF2', 'SIGNS_DIFFER', 'SCAN_CELL']
OPS = {name: k for k, name in enumerate(OP_NAMES)}
# columns an op reads and writes
N_IN = dict(SINCOS=1, EXP=1, EXP_BOUNDED=1, EXP_SMALL=1, CEXP=2, CEXP_BOUNDED=2, CEXP_PAIR=4, FRCP=1, FSQRT=1, FSQRT_HINV=1,
            CRECIP=2, CSQRT_FAST=2, CSQRT=2, CDIV=4, CMUL=4, CMADD=6, CMSUB=6, NEGATE_IF2=2, SIGNS_DIFFER=2, SCAN_CELL=2)
N_OUT = dict(SINCOS=2, EXP=1, EXP_BOUNDED=1, EXP_SMALL=1, CEXP=2, CEXP_BOUNDED=2, CEXP_PAIR=4, FRCP=1, FSQRT=1, FSQRT_HINV=2,
             CRECIP=2, CSQRT_FAST=2, CSQRT=2, CDIV=2, CMUL=2, CMADD=2, CMSUB=2, NEGATE_IF2=1, SIGNS_DIFFER=1, SCAN_CELL=2)
EXP_SMALL_BOUND = 0.34       # RF_EXP_SMALL, rf_core.h (test_math_probe.py checks it against the header)
_SIM = {}


def probe_sim():
    """g++ build of math_probe_sim.cpp with the device math of bh_math.h"""
    if 'hs' in _SIM:
        return _SIM['hs']
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so, src = os.path.join(d, 'libmath_probe_sim.so'), os.path.join(d, 'math_probe_sim.cpp')
    deps = [src] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', f)
                    for f in ('math_probe.h', 'bh_common.h', 'bh_math.h', 'rf_core.h', 'swd_core.h', 'swd_team.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        fma = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + fma + ['-o', so, src], check=True)
    hs = C.CDLL(so)
    hs.hs_math_probe.restype = C.c_int
    hs.hs_math_probe.argtypes = [C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    hs.hs_math_probe_nops.restype = C.c_int
    hs.hs_math_probe_exp_small_bound.restype = C.c_double
    hs.hs_std_complex.restype = None
    hs.hs_std_complex.argtypes = [C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    _SIM['hs'] = hs
    return hs


def pack(*cols):
    """[n][MP_IN] input block from up to six columns (the rest 0)"""
    cols = [np.asarray(c, dtype=np.float64).ravel() for c in cols]
    a = np.zeros((cols[0].size, MP_IN))
    for k, c in enumerate(cols):
        a[:, k] = c
    return a


def host(op, *cols):
    """op over the columns with the host build: the first N_OUT[op] output columns, [n][N_OUT]"""
    a = pack(*cols)
    out = np.full((a.shape[0], MP_OUT), 7.0)
    assert probe_sim().hs_math_probe(OPS[op], a.shape[0], a.ctypes.data, out.ctypes.data) == 0
    assert np.array_equal(out[:, N_OUT[op]:], np.zeros((a.shape[0], MP_OUT - N_OUT[op])))
    return out[:, :N_OUT[op]].copy()


def device(lib, op, *cols):
    """the same on the GPU (bh_selftest_math)"""
    from bayhunter_amd import _lib
    a = pack(*cols)
    out = np.full((a.shape[0], MP_OUT), 7.0)
    _lib.check(lib.bh_selftest_math(OPS[op], a.shape[0], a.ctypes.data, out.ctypes.data))
    assert np.array_equal(out[:, N_OUT[op]:], np.zeros((a.shape[0], MP_OUT - N_OUT[op])))
    return out[:, :N_OUT[op]].copy()


def std_complex(what, a):
    """g++'s std::complex<double> on [n][4] operands: what = 0 the quotient (a0 + i a1) / (a2 + i a3) -- libgcc's
    __divdc3 --, 1 std::sqrt(a0 + i a1) -- glibc's csqrt.  [n][2]"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros((a.shape[0], 2))
    probe_sim().hs_std_complex(what, a.shape[0], a.ctypes.data, out.ctypes.data)
    return out


def same_bits(a, b):
    """equal as int64 views wherever neither is NaN, and NaN in the same places"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


def count_different_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(np.int64) != b.view(np.int64)))).sum())


def ulp_err(got, ref):
    """|got - ref| in units of the spacing of doubles at |ref| (ref in long double), as test_math_accuracy measures it"""
    with np.errstate(invalid='ignore', over='ignore'):
        u = np.spacing(np.abs(ref.astype(np.float64)))
        return np.abs((np.asarray(got).astype(LD) - ref) / u).astype(np.float64)


# ---- sincos ------------------------------------------------------------------------------------------------------
INVPIO2 = 6.36619772367581382433e-01
SINCOS_SPECIAL = np.array([0.0, -0.0, 5e-324, 1e-300,
                           1e4, np.nextafter(1e4, 0), np.nextafter(1e4, np.inf), -1e4, np.nextafter(-1e4, 0), np.nextafter(-1e4, -np.inf),
                           1e12, np.nextafter(1e12, 0), np.inf, -np.inf, np.nan, -3e300])


def sincos_ties(n=10000, seed=21):
    """arguments whose x * 2/pi lies within 1e-9 of a half-integer: the tie of the quadrant's rint.  8 in 10 below 1e4
    (the one-step reduction), the rest up to 1e6 (the exact-product reduction)"""
    rs = np.random.RandomState(seed)
    nf = n * 8 // 10
    h = np.concatenate((rs.randint(-6366, 6366, nf), rs.randint(-636000, 636000, n - nf))) + 0.5
    return (h + rs.uniform(-0.8e-9, 0.8e-9, n)) * (np.pi / 2)


def sincos_segments(n_fast=200000, n_slow=120000, seed=0):
    """[(tag, arguments, ulp bound of test_math_accuracy)]: its three ranges, its three slow-path ranges with a third of
    each next to multiples of pi/2, and the ties"""
    rs = np.random.RandomState(seed)
    seg = []
    for lo, hi, bound in ((-1, 1, 0.85), (-300, 300, 0.85), (-1e4, 1e4, 1.1)):
        seg.append(('+-%g' % hi, rs.uniform(lo, hi, n_fast), bound))
    for lo, hi in ((1e4, 1.6e6), (1.6e6, 1e9), (1e9, 0.999e12)):
        x = rs.uniform(lo, hi, n_slow) * rs.choice([-1.0, 1.0], n_slow)
        m = n_slow // 3
        k = np.round(x[:m] / (np.pi / 2))
        x[:m] = np.nextafter(k * (np.pi / 2), np.inf) + k * 6.123233995736766e-17 * rs.choice([0, 1], m)
        seg.append(('%g..%g' % (lo, hi), x, 1.1))
    seg.append(('rint ties', sincos_ties(), 1.1))
    return seg


def sincos_ref(x):
    x = x.astype(LD)
    return np.sin(x), np.cos(x)


# ---- exp ---------------------------------------------------------------------------------------------------------
EXP_SPECIAL = np.array([0.0, -0.0, -745.5, -800, 710, 800, np.inf, -np.inf, np.nan])
EXP_BOUNDED_SPECIAL = np.array([1e6, -1e6, np.inf, -np.inf, np.nan])
EXP_SUBNORMAL = (-745.2, -708.0)


def exp_segments(n=400000, seed=1):
    """[(tag, arguments, ulp bound)]: the two ranges of test_math_accuracy"""
    rs = np.random.RandomState(seed)
    return [('%g..%g' % (lo, hi), rs.uniform(lo, hi, n), 0.95) for lo, hi in ((-60, 0), (-700, 700))]


def exp_subnormal_set(n=400000, seed=2):
    return np.random.RandomState(seed).uniform(EXP_SUBNORMAL[0], EXP_SUBNORMAL[1], n)


def exp_small_set():
    """the arguments of test_rf_floor.py::test_short_exponential_is_the_full_form_bit_for_bit"""
    rs = np.random.RandomState(3)
    b = EXP_SMALL_BOUND
    return np.concatenate(([0.0, -0.0, b, -b, np.nextafter(b, 0), -np.nextafter(b, 0), 5e-324, -5e-324, 1e-300, 1e-17],
                           rs.uniform(-b, b, 200000), rs.uniform(-1e-3, 1e-3, 20000), np.linspace(-b, b, 20001)))


def cexp_segments(n=200000, seed=4):
    """[(tag, re, im)]: re in (-60, 0) and in (-700, 700), im in (-300, 300)"""
    rs = np.random.RandomState(seed)
    return [('re %g..%g' % (lo, hi), rs.uniform(lo, hi, n), rs.uniform(-300.0, 300.0, n)) for lo, hi in ((-60, 0), (-700, 700))]


def cexp_ref(re, im):
    e = np.exp(re.astype(LD))
    return e * np.cos(im.astype(LD)), e * np.sin(im.astype(LD))


# bh_exp's 0.95 ulp for the modulus factor, sincos's 0.85 below 300, half an ulp for the product
CEXP_MODULUS_BOUND, CEXP_COMPONENT_BOUND = 0.95, 0.95 + 0.85 + 0.5


# ---- rf_cexp_pair in waves of 64 ------------------------------------------------------------------------------------
def _inside(rs, n):
    x = rs.uniform(-EXP_SMALL_BOUND, EXP_SMALL_BOUND, n)
    x[rs.rand(n) < 0.02] = EXP_SMALL_BOUND
    x[rs.rand(n) < 0.02] = -EXP_SMALL_BOUND
    return x


def _outside(rs, n):
    x = np.where(rs.rand(n) < 0.7, rs.uniform(-12.0, -EXP_SMALL_BOUND, n), rs.uniform(EXP_SMALL_BOUND, 1.0, n))
    x[rs.rand(n) < 0.02] = np.nextafter(EXP_SMALL_BOUND, 1.0)
    x[rs.rand(n) < 0.02] = -np.nextafter(EXP_SMALL_BOUND, 1.0)
    return x


WAVE_KINDS = ['inside', 'outside', 'lane0', 'lane31', 'lane63', 'nan']


def cexp_pair_waves(nwaves=16384, seed=5):
    """(za.re, za.im, zb.re, zb.im, kind[nwaves]) for nwaves waves of 64 elements.  kind: wholly inside |re| <= 0.34,
    wholly outside (each element has za.re, zb.re or both outside), exactly one lane outside at lane 0, 31 or 63, one NaN
    lane among lanes inside.  The first six waves are one of each kind."""
    rs = np.random.RandomState(seed)
    n = 64 * nwaves
    kind = np.concatenate((np.arange(6), rs.randint(0, 6, nwaves - 6)))
    ra, rb = _inside(rs, n).reshape(nwaves, 64), _inside(rs, n).reshape(nwaves, 64)
    oa, ob = _outside(rs, n).reshape(nwaves, 64), _outside(rs, n).reshape(nwaves, 64)
    which = rs.randint(0, 3, (nwaves, 64))                  # 0: za outside, 1: zb, 2: both
    lane = np.arange(64)[None, :]
    out = kind[:, None] == 1
    for k, l in ((2, 0), (3, 31), (4, 63)):
        out = out | ((kind[:, None] == k) & (lane == l))
    ra = np.where(out & (which != 1), oa, ra)
    rb = np.where(out & (which != 0), ob, rb)
    nanlane = rs.randint(0, 64, nwaves)[:, None]
    isnan = (kind[:, None] == 5) & (lane == nanlane)
    ra = np.where(isnan & (which != 1), np.nan, ra)
    rb = np.where(isnan & (which != 0), np.nan, rb)
    ia, ib = rs.uniform(-300.0, 300.0, n), rs.uniform(-300.0, 300.0, n)
    return ra.ravel(), ia, rb.ravel(), ib, kind


def pair_is_inside(ra, rb):
    with np.errstate(invalid='ignore'):
        return (np.abs(ra) <= EXP_SMALL_BOUND) & (np.abs(rb) <= EXP_SMALL_BOUND)


# ---- reciprocal and roots ------------------------------------------------------------------------------------------
def scaled_set(max_exp, n=1 << 19, seed=6, signed=False):
    """magnitudes 2^-max_exp .. 2^max_exp, the exponent uniform"""
    rs = np.random.RandomState(seed + max_exp)
    x = np.exp2(rs.uniform(-max_exp, max_exp, n))
    return x * rs.choice([-1.0, 1.0], n) if signed else x


def _mag(rs, n):
    return 10.0 ** rs.uniform(-6, 6, n) * rs.choice([-1.0, 1.0], n)


def complex_set(n=1 << 19, seed=7):
    """finite non-zero components of magnitude 1e-6 .. 1e6 (log-uniform, both signs)"""
    rs = np.random.RandomState(seed)
    return _mag(rs, n), _mag(rs, n)


def csqrt_fast_set(n=1 << 19, seed=8):
    """complex_set, then |im| = 1e-12 |re| on both signs of re and of im, then re = 0"""
    rs = np.random.RandomState(seed)
    re, im = _mag(rs, n), _mag(rs, n)
    m = n // 8
    re2 = _mag(rs, m)
    im2 = np.abs(re2) * 1e-12 * rs.choice([-1.0, 1.0], m)
    re3 = np.zeros(m) * rs.choice([-1.0, 1.0], m)            # +0 and -0
    return np.concatenate((re, re2, re3)), np.concatenate((im, im2, _mag(rs, m)))


def crecip_ref(re, im):
    re, im = re.astype(LD), im.astype(LD)
    d = re * re + im * im
    return re / d, -im / d


def csqrt_ref(re, im):
    """principal root in long double by the formula of csqrt_fast / csqrt_ (no cancelling sum): with m = sqrt((|z| +
    |re|) / 2) and o = im / (2 m), (m, o) for re > 0 and (|o|, copysign(m, im)) otherwise"""
    re, im = re.astype(LD), im.astype(LD)
    m = np.sqrt((np.sqrt(re * re + im * im) + np.abs(re)) * LD(0.5))
    o = im / (m + m)
    pos = re > 0
    return np.where(pos, m, np.abs(o)), np.where(pos, o, np.copysign(m, im))


def _polar(rs, n):
    m, ph = 10.0 ** rs.uniform(-6, 6, n), rs.uniform(-np.pi, np.pi, n)
    return m * np.cos(ph), m * np.sin(ph)


def cdiv_set(n=1 << 19, seed=9):
    """x.re, x.im, y.re, y.im: moduli 1e-6 .. 1e6 (log-uniform), phases uniform -- so that the quotient's phase is
    uniform too and few quotients have a component that is a cancelled sum (cdiv_well_conditioned)"""
    rs = np.random.RandomState(seed)
    return _polar(rs, n) + _polar(rs, n)


def cdiv_ref(a, b, c, d):
    a, b, c, d = (v.astype(LD) for v in (a, b, c, d))
    den = c * c + d * d
    return (a * c + b * d) / den, (b * c - a * d) / den


def cdiv_well_conditioned(a, b, c, d):
    """both components of the long-double quotient at least 1e-3 of its modulus"""
    qr, qi = cdiv_ref(a, b, c, d)
    mod = np.sqrt(qr * qr + qi * qi)
    return np.asarray((np.abs(qr) >= LD(1e-3) * mod) & (np.abs(qi) >= LD(1e-3) * mod))


# ---- fma chains, sign tests, scan cells --------------------------------------------------------------------------------
def fma_chain_set(ncols, n=1 << 20, seed=10):
    """ncols columns of magnitude 1e-6 .. 1e6, then rows with zeros of both signs, infinities, NaN and subnormals"""
    rs = np.random.RandomState(seed + ncols)
    cols = [_mag(rs, n) for _ in range(ncols)]
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -2.5e-310, 1e308, -1e308, 1.0])
    tail = rs.choice(odd, (4096, ncols))
    return [np.concatenate((c, tail[:, k])) for k, c in enumerate(cols)]


BITS_SPECIAL = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000,       # +-0, +-Inf
                         0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001,       # q/s NaN
                         0x7ff8dead0000beef, 0xfff4000000001234, 0x7fffffffffffffff, 0xffffffffffffffff,       # payloads
                         0x0000000000000001, 0x8000000000000001, 0x000fffffffffffff, 0x800fffffffffffff,       # subnormal
                         0x0010000000000000, 0x7fefffffffffffff, 0x3ff0000000000000, 0xbff0000000000000], dtype=np.uint64)


def bit_pattern_set(n=1 << 20, seed=12):
    """doubles of uniformly random bits -- every exponent, NaN payloads and subnormals among them -- after the list of
    special patterns"""
    rs = np.random.RandomState(seed)
    u = (rs.randint(0, 1 << 32, n).astype(np.uint64) << np.uint64(32)) | rs.randint(0, 1 << 32, n).astype(np.uint64)
    u[rs.rand(n) < 0.05] &= np.uint64(0x800fffffffffffff)                       # more subnormals and zeros
    u[rs.rand(n) < 0.05] |= np.uint64(0x7ff0000000000000)                       # more NaN and Inf
    return np.concatenate((BITS_SPECIAL, u)).view(np.float64)


def scan_cell_set():
    """the arguments of test_hostsim.py::test_scan_cells_in_closed_form_equal_repeated_addition and the reference's
    repeated addition of dc = dble(0.005): (base, cell, b, cn)"""
    rs = np.random.RandomState(3)
    n = 400000
    base = np.concatenate([rs.uniform(0.05, 9.0, n), rs.uniform(0.3, 5.3, n).astype(np.float32).astype(np.float64),
                           rs.choice([0.5, 1., 2., 4., 8.], n) - 0.35 * rs.rand(n) ** 2,
                           np.ldexp(rs.rand(n), rs.randint(-30, 10, n)), [0.0, -1.0, np.nan, np.inf]])
    cell = rs.randint(0, 64, base.size)
    dc = np.float64(np.float32(0.005))
    x, c = base.copy(), base + dc
    for k in range(1, 64):
        step = cell >= k
        x = np.where(step, c, x)
        c = np.where(step, x + dc, c)
    return base, cell, x, c
