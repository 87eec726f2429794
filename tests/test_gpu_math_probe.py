"""The device forms of the fp64 primitives of bh_math.h, bh_common.h, rf_core.h and swd_team.h, one call per element
(bh_selftest_math: the kernel of csrc/math_probe.hip over the op table of math_probe.h), about 2^20 elements per op.

A. Bit for bit against the host build of the same header (tests/hostsim/math_probe_sim.cpp, the other side of every
   #if defined(BH_HOSTSIM)): int64 views equal, NaN in the same places.  "The host replay is what the GPU computes" is
   the premise of every bit-for-bit test of the dispersion path; here it is checked per primitive, on the slow
   reduction, the NaN arm, saturation and subnormal results, the quadrant's rint tie and rf_cexp_pair's wave-uniform
   choice in waves with inactive lanes.
B. Accuracy of what has no host twin -- the v_rcp_f64 / v_rsq_f64 sequences frcp, fsqrt, fsqrt_hinv, crecip,
   csqrt_fast, the contracted csqrt_ and the complex quotient -- against long double (64 significant bits).

Every test prints its worst figure before it asserts.  Measured on an MI355X: DESIGN.md sections 4.1 and 4.2 have the figures."""
import numpy as np
import pytest

import math_probe_cases as mc
from math_probe_cases import LD, device, host, same_bits, ulp_err

pytestmark = pytest.mark.gpu


def _bits(tag, got, want):
    bad = mc.count_different_bits(got, want)
    print('gpu math_probe, %s: %d of %d values differ from the host build' % (tag, bad, np.asarray(got).size))
    assert same_bits(got, want), (tag, bad)


# ---- sincos ------------------------------------------------------------------------------------------------------
def test_sincos_equals_the_host_build_and_keeps_its_bounds(lib):
    seg = mc.sincos_segments()
    x = np.concatenate([s[1] for s in seg] + [mc.SINCOS_SPECIAL])
    got = device(lib, 'SINCOS', x)
    ws, wc = mc.sincos_ref(x)
    lo = 0
    figures = []
    for tag, xs, bound in seg:
        sl = slice(lo, lo + xs.size)
        lo += xs.size
        worst = max(ulp_err(got[sl, 0], ws[sl]).max(), ulp_err(got[sl, 1], wc[sl]).max())
        print('gpu math_probe, SINCOS %s: worst %.3f ulp (bound %.2f)' % (tag, worst, bound))
        figures.append((tag, worst, bound))
    sp = got[lo:]
    assert np.isfinite(sp[:12]).all(axis=1).sum() == 11 and np.isnan(sp[10]).all() and np.isnan(sp[12:]).all()
    assert sp[0, 0] == 0 and sp[1, 0] == 0 and not np.signbit(sp[:2, 0]).any() and (sp[:4, 1] == 1.0).all()
    _bits('SINCOS', got, host('SINCOS', x))
    for tag, worst, bound in figures:
        assert worst <= bound, (tag, worst)


# ---- exp ---------------------------------------------------------------------------------------------------------
def test_exp_equals_the_host_build_and_keeps_its_bounds(lib):
    seg = mc.exp_segments()
    sub = mc.exp_subnormal_set(200000)
    x = np.concatenate([s[1] for s in seg] + [sub, mc.EXP_SPECIAL])
    got = device(lib, 'EXP', x)[:, 0]
    lo = 0
    figures = []
    for tag, xs, bound in seg:
        sl = slice(lo, lo + xs.size)
        lo += xs.size
        figures.append((tag, ulp_err(got[sl], np.exp(xs.astype(LD))).max(), bound))
    ref = np.exp(sub.astype(LD))
    gs = got[lo:lo + sub.size]
    figures.append(('subnormal results', float((np.abs(gs.astype(LD) - ref) / np.spacing(ref.astype(np.float64)).astype(LD)).max()), 1.0))
    for tag, worst, bound in figures:
        print('gpu math_probe, EXP %s: worst %.3f ulp (bound %.2f)' % (tag, worst, bound))
    with np.errstate(over='ignore'):
        assert same_bits(got[lo + sub.size:], np.exp(mc.EXP_SPECIAL))
    _bits('EXP', got, host('EXP', x)[:, 0])
    for tag, worst, bound in figures:
        assert worst <= bound, (tag, worst)


def test_exp_bounded_and_exp_small_equal_the_host_build(lib):
    seg = mc.exp_segments()
    small = mc.exp_small_set()
    x = np.concatenate([s[1] for s in seg] + [small, mc.EXP_SPECIAL, mc.EXP_BOUNDED_SPECIAL])
    got = device(lib, 'EXP_BOUNDED', x)[:, 0]
    lo = 0
    figures = []
    for tag, xs, bound in seg:
        figures.append(('EXP_BOUNDED ' + tag, ulp_err(got[lo:lo + xs.size], np.exp(xs.astype(LD))).max(), bound))
        lo += xs.size
    gs = device(lib, 'EXP_SMALL', small)[:, 0]
    figures.append(('EXP_SMALL |x| <= 0.34', ulp_err(gs, np.exp(small.astype(LD))).max(), 1.0))
    for tag, worst, bound in figures:
        print('gpu math_probe, %s: worst %.3f ulp (bound %.2f)' % (tag, worst, bound))
    tail = got[lo + small.size + mc.EXP_SPECIAL.size:]
    assert tail[0] == np.inf and tail[1] == 0.0 and not np.signbit(tail[1]) and np.isnan(tail[2:]).all()      # ldexp saturates
    _bits('EXP_BOUNDED', got, host('EXP_BOUNDED', x)[:, 0])
    _bits('EXP_SMALL', gs, host('EXP_SMALL', small)[:, 0])
    # inside its bound the short form is the full form on the device too
    assert np.array_equal(gs.view(np.int64), got[lo:lo + small.size].view(np.int64))
    for tag, worst, bound in figures:
        assert worst <= bound, (tag, worst)


@pytest.mark.parametrize('op', ['CEXP', 'CEXP_BOUNDED'])
def test_cexp_equals_the_host_build(lib, op):
    seg = mc.cexp_segments(1 << 19)
    re_ = np.concatenate([s[1] for s in seg] + [[0.0, -np.inf, 800.0, 0.0, np.nan, 0.0, 1e6, -1e6]])
    im = np.concatenate([s[2] for s in seg] + [[0.0, 0.0, 0.0, np.inf, 0.0, 1e12, 0.0, 1.0]])
    got = device(lib, op, re_, im)
    wr, wi = mc.cexp_ref(re_[:-8], im[:-8])
    worst = max(ulp_err(got[:-8, 0], wr).max(), ulp_err(got[:-8, 1], wi).max())
    print('gpu math_probe, %s: worst component %.3f ulp against long double' % (op, worst))
    _bits(op, got, host(op, re_, im))


# ---- rf_cexp_pair: the wave-uniform choice of the exponential's form ----------------------------------------------------
def test_cexp_pair_does_not_depend_on_the_wave(lib):
    """Waves of 64 elements (thread i handles element i, math_probe.h): wholly inside |re| <= 0.34 (the short form), wholly
    outside, exactly one lane outside at lane 0, 31 or 63, one NaN lane.  Each output is cexp_bounded of its own argument
    whatever the other 63 lanes hold; a prefix of whole waves run alone gives the bits it gives inside the full array;
    and a last wave of 1 or 63 active lanes, all inside, next to elements outside that a kernel without its `i < n`
    guard would take into the wave (behind them the device buffer's padding is NaN: outside as well)."""
    ra, ia, rb, ib, kind = mc.cexp_pair_waves()
    n = ra.size
    assert n == 1 << 20
    got = device(lib, 'CEXP_PAIR', ra, ia, rb, ib)
    fa, fb = host('CEXP_BOUNDED', ra, ia), host('CEXP_BOUNDED', rb, ib)
    for k, name in enumerate(mc.WAVE_KINDS):
        w = np.repeat(kind == k, 64)
        bad = mc.count_different_bits(got[w, :2], fa[w]) + mc.count_different_bits(got[w, 2:], fb[w])
        print('gpu math_probe, CEXP_PAIR waves "%s": %d of %d values differ from cexp_bounded (host build)' % (name, bad, 4 * w.sum()))
    assert same_bits(got[:, :2], fa) and same_bits(got[:, 2:], fb)
    assert same_bits(got[:, :2], device(lib, 'CEXP_BOUNDED', ra, ia)) and same_bits(got[:, 2:], device(lib, 'CEXP_BOUNDED', rb, ib))
    assert same_bits(got, host('CEXP_PAIR', ra, ia, rb, ib))
    for waves in (1, 6, 7, 1000):
        m = 64 * waves
        assert same_bits(device(lib, 'CEXP_PAIR', ra[:m], ia[:m], rb[:m], ib[:m]), got[:m]), waves
    # partial last waves: lanes 0 .. active-1 of the wave inside, every later element of the array outside
    inside = np.flatnonzero(kind == 0)[:2]
    outside = np.flatnonzero(kind == 1)[:2]
    for active, wi, wo in ((1, inside[0], outside[0]), (63, inside[1], outside[1])):
        cols = []
        for v in (ra, ia, rb, ib):
            last = np.concatenate((v[64 * wi:64 * wi + active], v[64 * wo + active:64 * wo + 64]))
            cols.append(np.concatenate((v[:64 * 5], last)))
        m = 64 * 5 + active
        assert mc.pair_is_inside(cols[0][320:m], cols[2][320:m]).all() and not mc.pair_is_inside(cols[0][m:], cols[2][m:]).any()
        part = device(lib, 'CEXP_PAIR', *[c[:m] for c in cols])
        want = np.concatenate((host('CEXP_BOUNDED', cols[0][:m], cols[1][:m]), host('CEXP_BOUNDED', cols[2][:m], cols[3][:m])), axis=1)
        assert part.shape == (m, 4) and same_bits(part, want), active
        assert same_bits(device(lib, 'CEXP_PAIR', *cols)[:m], part), active


# ---- fma chains, sign tricks, scan cells ----------------------------------------------------------------------------
@pytest.mark.parametrize('op', ['CMUL', 'CMADD', 'CMSUB'])
def test_explicit_fma_chains_equal_the_host_build(lib, op):
    cols = mc.fma_chain_set(mc.N_IN[op])
    with np.errstate(all='ignore'):
        _bits(op, device(lib, op, *cols), host(op, *cols))


def test_sign_bit_forms_equal_the_host_forms(lib):
    x = mc.bit_pattern_set()
    two = 2.0 * (np.arange(x.size) % 2)
    got = device(lib, 'NEGATE_IF2', x, two)[:, 0]
    want = np.where(two != 0, -x, x)
    bad = int((got.view(np.int64) != want.view(np.int64)).sum())
    print('gpu math_probe, NEGATE_IF2: %d of %d bit patterns differ from -x / x' % (bad, x.size))
    assert bad == 0 and np.array_equal(got.view(np.int64), host('NEGATE_IF2', x, two)[:, 0].view(np.int64))   # payloads too
    y = mc.bit_pattern_set(seed=13)
    got = device(lib, 'SIGNS_DIFFER', x, y)[:, 0]
    assert np.array_equal(got, (np.signbit(x) != np.signbit(y)).astype(np.float64))
    assert np.array_equal(got, host('SIGNS_DIFFER', x, y)[:, 0])


def test_scan_cells_equal_repeated_addition_on_the_device(lib):
    base, cell, b, cn = mc.scan_cell_set()
    got = device(lib, 'SCAN_CELL', base, cell)
    _bits('SCAN_CELL', got, host('SCAN_CELL', base, cell))
    assert same_bits(got, np.stack((b, cn), axis=1))


# ---- B: the hardware-seeded sequences against long double --------------------------------------------------------------
# bh_common.h claimed "~1 ulp" for frcp, fsqrt and fsqrt_hinv.  The bound is that claim, 1 ulp (measured: 0.500 for
# frcp, fsqrt and the root of fsqrt_hinv on both ranges) -- except for h of fsqrt_hinv: once its last Newton step was
# mended (it took half the correction: 10.04 / 9.99 ulp on the two ranges, and 18.7 ulp in csqrt_fast) it measures 1.480
# and 1.486 ulp, above the claim and below 2, so the comment now says so and the bound is the measurement rounded up to
# the next quarter ulp.  (0.5 / sqrt(x), the host stand-in with its two roundings, measures 1.480 / 1.486 as well.)
SEQ_BOUND = 1.0
HINV_H_BOUND = 1.5


@pytest.mark.parametrize('max_exp', [20, 300])
def test_reciprocal_and_root_sequences(lib, max_exp):
    """frcp (both signs), fsqrt and both outputs of fsqrt_hinv for magnitudes 2^-20 .. 2^20 (the "well scaled" range of
    their comment) and 2^-300 .. 2^300; NaN in, NaN out."""
    xr = np.concatenate((mc.scaled_set(max_exp, signed=True), [np.nan]))
    xs = np.concatenate((mc.scaled_set(max_exp), [np.nan]))
    r = device(lib, 'FRCP', xr)[:, 0]
    g = device(lib, 'FSQRT', xs)[:, 0]
    gh = device(lib, 'FSQRT_HINV', xs)
    root = np.sqrt(xs[:-1].astype(LD))
    figures = [('FRCP', ulp_err(r[:-1], 1 / xr[:-1].astype(LD)).max(), SEQ_BOUND), ('FSQRT', ulp_err(g[:-1], root).max(), SEQ_BOUND),
               ('FSQRT_HINV g', ulp_err(gh[:-1, 0], root).max(), SEQ_BOUND),
               ('FSQRT_HINV h', ulp_err(gh[:-1, 1], LD(0.5) / root).max(), HINV_H_BOUND)]
    for tag, worst, bound in figures:
        print('gpu math_probe, %s 2^+-%d: worst %.3f ulp (bound %.2f)' % (tag, max_exp, worst, bound))
    assert np.isnan(r[-1]) and np.isnan(g[-1]) and np.isnan(gh[-1]).all()
    assert not np.isnan(r[:-1]).any() and not np.isnan(g[:-1]).any() and not np.isnan(gh[:-1]).any()
    for tag, worst, bound in figures:
        assert worst <= bound, (tag, worst)


def test_crecip_against_long_double(lib):
    """1/z = conj(z) frcp(re^2 + im^2), components of magnitude 1e-6 .. 1e6.  Bound, half an ulp per rounded operation
    and one for frcp (the bound of test_reciprocal_and_root_sequences): re^2, im^2 and their sum 1.5 -- a sum of
    positive terms, no cancellation --, frcp 1, the product with re or im 0.5: 3 ulp per component.  (Contraction
    fuses one product into the sum on the device: one rounding fewer, the bound stands.)"""
    re_, im = mc.complex_set(1 << 20)
    got = device(lib, 'CRECIP', re_, im)
    wr, wi = mc.crecip_ref(re_, im)
    worst = max(ulp_err(got[:, 0], wr).max(), ulp_err(got[:, 1], wi).max())
    print('gpu math_probe, CRECIP: worst component %.3f ulp (bound 3)' % worst)
    assert np.array_equal(np.signbit(got[:, 0]), re_ < 0) and np.array_equal(np.signbit(got[:, 1]), im > 0)
    assert worst <= 3.0


def test_csqrt_fast_against_long_double(lib):
    """The principal root for im != 0: d = fsqrt(re^2 + im^2), (m, h) = fsqrt_hinv((d + |re|) / 2), o = im h.  Bound, half
    an ulp per rounded operation and one per fsqrt / fsqrt_hinv output: re^2, im^2, their sum 1.5; fsqrt 1; d + |re| 0.5
    (the halving is exact); fsqrt_hinv 1: 4 ulp for m -- counting the error of the root's argument in full, where the root
    halves it --, and o = im h has h's error and a product's 0.5 where m has none after its root: with the halving, 1.5 +
    1 + 0.5 = 3 ulp, so 4 holds for both.  No sum cancels: d + |re| adds positive terms.  Also |im| = 1e-12 |re| on both
    signs of re, and re = +-0.  The branch is the principal one: real part >= 0, the imaginary part's sign is im's.
    Measured: 2.64 ulp (17.9 before fsqrt_hinv's last step was mended)."""
    re_, im = mc.csqrt_fast_set(1 << 20)
    got = device(lib, 'CSQRT_FAST', re_, im)
    wr, wi = mc.csqrt_ref(re_, im)
    err = np.maximum(ulp_err(got[:, 0], wr), ulp_err(got[:, 1], wi))
    n = 1 << 20
    for tag, sl in (('generic', slice(0, n)), ('|im| = 1e-12 |re|', slice(n, n + n // 8)), ('re = 0', slice(n + n // 8, None))):
        print('gpu math_probe, CSQRT_FAST %s: worst component %.3f ulp (bound 4)' % (tag, err[sl].max()))
    assert (got[:, 0] >= 0).all() and not np.signbit(got[:, 0]).any() and np.array_equal(np.signbit(got[:, 1]), im < 0)
    assert err.max() <= 4.0


def test_contracted_csqrt_stays_next_to_the_host_build(lib):
    """csqrt_ is compiled with fp contraction on the device (bh_common.h: re^2 + im^2 becomes one fma), so it is not
    bit-equal to the host build; it has no cancelling sum: within 2 ulp of the host build's value, componentwise."""
    re_, im = mc.complex_set()
    got, want = device(lib, 'CSQRT', re_, im), host('CSQRT', re_, im)
    worst = max(ulp_err(got[:, k], want[:, k].astype(LD)).max() for k in (0, 1))
    print('gpu math_probe, CSQRT device against host build: worst component %.3f ulp (bound 2), %.2f %% of values differ'
          % (worst, 100.0 * mc.count_different_bits(got, want) / got.size))
    assert worst <= 2.0


def test_quotient_stays_next_to_the_host_build(lib):
    """The complex quotient (Smith's algorithm, libgcc's __divdc3) on the device against the host build.  Quotients with
    a component below 1e-3 of the modulus in long double are left out (0.12 % of the set,
    test_math_probe.py::test_cdiv_set_is_well_conditioned); the others within 2 ulp of the host build's value,
    componentwise.

    With the products of the quotient fused on the device (fp contraction, as the rest of the complex arithmetic has
    it) this measured 272 ulp at worst over the 523 639 quotients kept, 4.72 % of them above 2 ulp, 104 172 ulp over all
    524 288 and 4.03 ulp of the modulus: Smith's numerator a (c/d) + b cancels -- a component at 1e-3 of the modulus is
    a sum cancelled a thousandfold -- and a fused product changes what is left.  A contracted g++ build of the same
    source gave the same figures.  The quotient is now compiled without contraction (bh_common.h): every operation is
    then an IEEE operation on both sides, so the device must give the host build's bits on the whole set, the
    cancelled quotients included; that is asserted too."""
    a, b, c, d = mc.cdiv_set()
    keep = mc.cdiv_well_conditioned(a, b, c, d)
    assert keep.mean() >= 0.98
    got, want = device(lib, 'CDIV', a, b, c, d), host('CDIV', a, b, c, d)
    err = np.maximum(ulp_err(got[:, 0], want[:, 0].astype(LD)), ulp_err(got[:, 1], want[:, 1].astype(LD)))
    qr, qi = mc.cdiv_ref(a, b, c, d)
    exact = np.maximum(ulp_err(got[:, 0], qr), ulp_err(got[:, 1], qi))
    hexact = np.maximum(ulp_err(want[:, 0], qr), ulp_err(want[:, 1], qi))
    mod = np.sqrt(qr * qr + qi * qi)
    emod = (np.sqrt((got[:, 0].astype(LD) - want[:, 0]) ** 2 + (got[:, 1].astype(LD) - want[:, 1]) ** 2)
            / np.spacing(mod.astype(np.float64))).astype(np.float64)
    print('gpu math_probe, CDIV device against host build: worst component %.3f ulp (bound 2) over %d quotients kept, %.2f %% of '
          'them above 2; %.3f over all; in ulp of the modulus %.3f over all; against long double: device %.3f, host build %.3f '
          'over those kept' % (err[keep].max(), keep.sum(), 100 * (err[keep] > 2).mean(), err.max(), emod.max(),
                               exact[keep].max(), hexact[keep].max()))
    print('gpu math_probe, CDIV: %d of %d values differ from the host build' % (mc.count_different_bits(got, want), got.size))
    assert err[keep].max() <= 2.0
    assert same_bits(got, want)
