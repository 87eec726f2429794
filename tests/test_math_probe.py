"""CPU tier of the math probe: the host forms of the primitives of bh_math.h, bh_common.h, rf_core.h and swd_team.h through
the op table of csrc/math_probe.h (tests/hostsim/math_probe_sim.cpp, device math), where the suite did not reach them,
and the input sets that tests/test_gpu_math_probe.py runs on the device.  Each test prints its worst figure before it
asserts.

Special values of the host build (test_special_values asserts every line; anything else finite and in an op's stated
domain gives no NaN, test_no_nan_inside_the_domains):

    SINCOS        0 -> (+0, 1); -0 -> (+0, 1): sin(-0) is +0, not -0 (the reduction's fma(-fn, PIO2_1, x) adds +0 to -0);
                  5e-324 -> (5e-324, 1); the largest double below 1e12 -> finite; 1e12, +-Inf, NaN, -3e300 -> (NaN, NaN)
    EXP           +-0 -> 1; -745.5, -800, -Inf -> +0; 710, 800, +Inf -> +Inf; NaN -> NaN
    EXP_BOUNDED   +-0 -> 1; 1e6 -> +Inf; -1e6 -> +0; +-Inf -> NaN (the reduction's Inf - Inf; exp gives Inf / 0); NaN -> NaN
    EXP_SMALL     +-0 -> 1; NaN -> NaN
    CEXP          (0, 0) -> (1, +0); (-Inf, 0) -> (+0, +0); (800, 0) -> (+Inf, NaN): Inf * sin 0, where glibc's cexp gives
                  (+Inf, 0); (0, Inf), (NaN, 0), (0, 1e12) -> (NaN, NaN)
    CEXP_BOUNDED  (0, 0) -> (1, +0); (1e6, 0) -> (+Inf, NaN); (-1e6, 1) -> (+0, +0); (-Inf, 0), (0, Inf) -> (NaN, NaN)
    CEXP_PAIR     each output as CEXP_BOUNDED of its argument
    FRCP          (host: 1 / x)  +-0 -> +-Inf; +-Inf -> +-0; NaN -> NaN
    FSQRT         (host: sqrt)   +-0 -> +-0; +Inf -> +Inf; -1 -> NaN; NaN -> NaN
    FSQRT_HINV    (host: sqrt, 0.5 / root)  +0 -> (+0, +Inf); +Inf -> (+Inf, +0); -1, NaN -> (NaN, NaN)
    CRECIP        (0, 0) -> (NaN, NaN): outside its domain (z != 0); (2, 0) -> (0.5, -0)
    CSQRT_FAST    (0, 0) -> (NaN, +0): outside its domain (im != 0); (4, 0) -> (2, +0); (-4, 0) -> (+0, 2); (-4, -0) -> (+0, -2)
    CSQRT         (0, 0) -> (+0, +0); (-4, 0) -> (+0, 2); (-4, -0) -> (+0, -2); (0, 2) -> (1, 1); (NaN, 1) -> (NaN, NaN)
    CDIV          y = (0, 0) -> (NaN, NaN) (Smith's ratio 0 / 0; no recovery tail); (1, 1) / (1, 1) -> (1, +0)
    CMUL / CMADD / CMSUB   NaN only from a NaN operand, Inf * 0 or Inf - Inf
    NEGATE_IF2    the sign bit flipped or not, every other bit kept: NaN in, NaN out
    SIGNS_DIFFER  0 or 1 for every pair, NaN included
    SCAN_CELL     NaN base -> (NaN, NaN); +Inf -> (+Inf, +Inf)
"""
import re
import os

import numpy as np

import math_probe_cases as mc
from math_probe_cases import LD, host, same_bits, ulp_err

INF, NAN = np.inf, np.nan


def test_op_table_matches_the_header():
    txt = open(os.path.join(mc.ROOT, 'bayhunter_amd', 'csrc', 'math_probe.h')).read()
    body = txt[txt.index('enum MathProbeOp'):txt.index('MP_NOPS')]
    names = re.findall(r'^\s*MP_([A-Z0-9_]+)\b', body, flags=re.M)
    assert names == mc.OP_NAMES and mc.probe_sim().hs_math_probe_nops() == len(names)
    assert mc.probe_sim().hs_math_probe_exp_small_bound() == mc.EXP_SMALL_BOUND
    assert set(mc.N_IN) == set(mc.N_OUT) == set(names)
    bad = np.zeros((1, 6))
    out = np.zeros((1, 4))
    for op in (-1, len(names)):
        assert mc.probe_sim().hs_math_probe(op, 1, bad.ctypes.data, out.ctypes.data) == 1


def test_exp_bounded_and_cexp_against_long_double():
    """exp / cexp in long double on (-60, 0) and (-700, 700) x (-300, 300).  The modulus factor gets bh_exp's 0.95 ulp; a
    component that plus sincos's 0.85 plus half an ulp for the product: 2.3.  That sum of ulps is a count, not a strict
    bound (an ulp of a factor can weigh up to two ulp of the product): 200 000 draws per range reach 2.24, the 2^19 draws
    of the GPU tier 2.31, on the device and in this build alike."""
    for tag, x, bound in mc.exp_segments():
        worst = ulp_err(host('EXP_BOUNDED', x)[:, 0], np.exp(x.astype(LD))).max()
        print('math_probe host: EXP_BOUNDED %s worst %.3f ulp (bound %.2f)' % (tag, worst, bound))
        assert worst <= bound
    for op in ('CEXP', 'CEXP_BOUNDED'):
        for tag, re_, im in mc.cexp_segments():
            got = host(op, re_, im)
            wr, wi = mc.cexp_ref(re_, im)
            wc = max(ulp_err(got[:, 0], wr).max(), ulp_err(got[:, 1], wi).max())
            print('math_probe host: %s %s worst component %.3f ulp (bound %.2f)' % (op, tag, wc, mc.CEXP_COMPONENT_BOUND))
            assert wc <= mc.CEXP_COMPONENT_BOUND
            # the modulus factor e^re is what the op returns at im = 0 (cos 0 = 1, sin 0 = +0)
            e0 = host(op, re_, np.zeros_like(re_))
            wm = ulp_err(e0[:, 0], np.exp(re_.astype(LD))).max()
            print('math_probe host: %s %s modulus factor worst %.3f ulp (bound %.2f)' % (op, tag, wm, mc.CEXP_MODULUS_BOUND))
            assert wm <= mc.CEXP_MODULUS_BOUND and np.all(e0[:, 1] == 0.0)


def test_exp_in_the_subnormal_range():
    """bh_exp's results below 2^-1022, x in (-745.2, -708): one rounding of ldexp into the subnormal range behind the
    polynomial's.  Within one spacing of the long-double value; measured with this host build: worst 0.873 of 400 000
    draws, 99.0 % of them equal to glibc's exp."""
    x = mc.exp_subnormal_set()
    got = host('EXP', x)[:, 0]
    ref = np.exp(x.astype(LD))
    assert (got < 2.2250738585072014e-308).mean() > 0.97 and got.min() >= 0.0
    err = np.abs(got.astype(LD) - ref) / np.spacing(ref.astype(np.float64)).astype(LD)
    same = (got == np.exp(x)).mean()
    print('math_probe host: EXP subnormal results worst %.3f spacings, %.1f %% equal to glibc' % (err.max(), 100 * same))
    assert err.max() <= 1.0 and same >= 0.98


def test_csqrt_is_glibcs_formulation_with_a_plain_modulus():
    """csqrt_ against numpy's complex128 sqrt (glibc's csqrt; std::sqrt of g++ gives the same bits).  The library only
    calls it with im == 0 (the vertical slownesses of rf_coeffm): bit-equal there and at re == 0.  For generic arguments
    it is glibc's formulation except that |z| is sqrt(re^2 + im^2) where glibc takes hypot(re, im), which differs in the
    last bit for 15 % of these operands; the root differs for 5.7 % of them and only there.  A one-ulp step of the modulus
    moves the larger root by at most one ulp and the quotient by it, the other component, by at most one more: two ulp
    (measured: 2.00).  Either formulation is reproduced bit for bit with its modulus, so that is the whole difference."""
    re_, im = mc.complex_set()
    got = host('CSQRT', re_, im)
    z = re_ + 1j * im
    want = np.sqrt(z)
    assert same_bits(mc.std_complex(1, np.stack((re_, im, re_, im), axis=1)), np.stack((want.real, want.imag), axis=1))
    plain, hyp = np.sqrt(re_ * re_ + im * im), np.hypot(re_, im)
    differs = (got[:, 0] != want.real) | (got[:, 1] != want.imag)
    worst = max(ulp_err(got[:, 0], want.real.astype(LD)).max(), ulp_err(got[:, 1], want.imag.astype(LD)).max())
    print('math_probe host: CSQRT differs from glibc for %.2f %% of %d (modulus differs for %.2f %%), worst %.2f ulp'
          % (100 * differs.mean(), re_.size, 100 * (plain != hyp).mean(), worst))
    assert not (differs & (plain == hyp)).any() and worst <= 2.0
    for d, ref in ((plain, got), (hyp, np.stack((want.real, want.imag), axis=1))):
        pos = re_ > 0
        big = np.sqrt(0.5 * (d + np.abs(re_)))
        small = 0.5 * (im / big)
        r, s = np.where(pos, big, np.abs(small)), np.copysign(np.where(pos, small, big), im)
        assert same_bits(np.stack((r, s), axis=1), ref)
    # the arguments the library passes, and the other axis
    x = np.concatenate((re_, [0.0, 4.0, -4.0]))
    for a, b in ((x, np.zeros_like(x)), (x, -np.zeros_like(x)), (np.zeros_like(x), x), (-np.zeros_like(x), x)):
        z = np.empty(a.size, dtype=np.complex128)                # (a + 1j * b loses the sign of a zero b)
        z.real, z.imag = a, b
        w = np.sqrt(z)
        assert same_bits(host('CSQRT', a, b), np.stack((w.real, w.imag), axis=1))


def test_cdiv_is_libgccs_quotient():
    """operator/(cd, cd) against g++'s std::complex quotient (libgcc's __divdc3, what the reference's division lowers
    to): bit-equal.  numpy's complex128 `/` is not libgcc's: its loop multiplies the numerators by the rounded reciprocal
    of Smith's denominator instead of dividing by it -- one rounding more, up to one ulp per component, for four in ten of
    the quotients.  Both are reproduced bit for bit here, so that is the whole difference."""
    a, b, c, d = mc.cdiv_set()
    got = host('CDIV', a, b, c, d)
    assert same_bits(got, mc.std_complex(0, np.stack((a, b, c, d), axis=1)))
    q = (a + 1j * b) / (c + 1j * d)
    big = np.abs(c) >= np.abs(d)
    rat = np.where(big, d / c, c / d)
    nr, ni = np.where(big, b * rat + a, a * rat + b), np.where(big, b - a * rat, b * rat - a)
    den = np.where(big, d * rat + c, c * rat + d)
    assert same_bits(got, np.stack((nr / den, ni / den), axis=1))
    scl = 1.0 / den
    assert same_bits(np.stack((q.real, q.imag), axis=1), np.stack((nr * scl, ni * scl), axis=1))
    worst = max(ulp_err(got[:, 0], q.real.astype(LD)).max(), ulp_err(got[:, 1], q.imag.astype(LD)).max())
    share = ((got[:, 0] != q.real) | (got[:, 1] != q.imag)).mean()
    print('math_probe host: CDIV differs from numpy for %.1f %% of %d quotients, worst %.2f ulp' % (100 * share, a.size, worst))
    assert worst <= 1.0


def test_cdiv_set_is_well_conditioned():
    """The GPU tier compares the contracted device quotient with this build componentwise, except where a component of
    the long-double quotient is below 1e-3 of its modulus (a cancelled sum): at most 2 % of the set may be excluded."""
    ok = mc.cdiv_well_conditioned(*mc.cdiv_set())
    print('math_probe: CDIV set, %.3f %% of %d quotients excluded' % (100 * (1 - ok.mean()), ok.size))
    assert 1 - ok.mean() <= 0.02
    for v in mc.cdiv_set() + mc.complex_set():
        assert np.isfinite(v).all() and (v != 0).all()
    for v in (np.hypot(*mc.cdiv_set()[:2]), np.hypot(*mc.cdiv_set()[2:])) + tuple(np.abs(v) for v in mc.complex_set()):
        assert v.min() >= 1e-6 and v.max() <= 1e6


def test_input_sets():
    """What the GPU tier relies on in its inputs."""
    x = mc.sincos_ties()
    t = x.astype(LD) * LD(mc.INVPIO2)
    assert x.size == 10000 and np.abs(t - np.floor(t) - LD(0.5)).max() < 1e-9
    assert (np.abs(x) < 1e4).sum() >= 7900 and (np.abs(x) >= 1e4).sum() >= 1900
    # the tie is real: both neighbouring quadrants are taken
    fn = np.rint(x * mc.INVPIO2)
    assert 0.3 < (fn > x * mc.INVPIO2).mean() < 0.7
    seg = mc.sincos_segments()
    assert sum(s[1].size for s in seg) + mc.SINCOS_SPECIAL.size > 900000
    assert max(np.abs(s[1]).max() for s in seg) < 1e12
    ra, ia, rb, ib, kind = mc.cexp_pair_waves(1024)
    inside = mc.pair_is_inside(ra, rb).reshape(-1, 64)
    nan = (np.isnan(ra) | np.isnan(rb)).reshape(-1, 64)
    assert set(kind) == set(range(6)) and list(kind[:6]) == list(range(6))
    assert inside[kind == 0].all() and not inside[kind == 1].any()
    for k, lane in ((2, 0), (3, 31), (4, 63)):
        w = inside[kind == k]
        assert not w[:, lane].any() and w.sum(axis=1).tolist() == [63] * w.shape[0]
    assert (nan[kind == 5].sum(axis=1) == 1).all() and not nan[kind != 5].any()
    assert (inside[kind == 5].sum(axis=1) == 63).all()
    assert (np.abs(ra) == mc.EXP_SMALL_BOUND).any() and (np.abs(ra) == np.nextafter(mc.EXP_SMALL_BOUND, 1)).any()
    assert mc.exp_small_set().size == 240011 and np.abs(mc.exp_small_set()).max() == mc.EXP_SMALL_BOUND
    re_, im = mc.csqrt_fast_set()
    assert (im != 0).all() and np.isfinite(re_).all() and (re_ == 0).sum() == (1 << 16)
    tiny = np.abs(im) < 1e-11 * np.abs(re_)
    assert (tiny & (re_ > 0) & (im > 0)).any() and (tiny & (re_ > 0) & (im < 0)).any()
    assert (tiny & (re_ < 0) & (im > 0)).any() and (tiny & (re_ < 0) & (im < 0)).any()
    b = mc.bit_pattern_set()
    assert np.isnan(b).mean() > 0.03 and (np.abs(b) < 2.3e-308).mean() > 0.03 and np.isinf(b).any()


SPECIAL = [
    ('SINCOS', (0.0,), (0.0, 1.0)), ('SINCOS', (-0.0,), (0.0, 1.0)), ('SINCOS', (5e-324,), (5e-324, 1.0)),
    ('SINCOS', (1e12,), (NAN, NAN)), ('SINCOS', (INF,), (NAN, NAN)), ('SINCOS', (-INF,), (NAN, NAN)),
    ('SINCOS', (NAN,), (NAN, NAN)), ('SINCOS', (-3e300,), (NAN, NAN)),
    ('EXP', (0.0,), (1.0,)), ('EXP', (-0.0,), (1.0,)), ('EXP', (-745.5,), (0.0,)), ('EXP', (-800.0,), (0.0,)),
    ('EXP', (-INF,), (0.0,)), ('EXP', (710.0,), (INF,)), ('EXP', (800.0,), (INF,)), ('EXP', (INF,), (INF,)), ('EXP', (NAN,), (NAN,)),
    ('EXP_BOUNDED', (0.0,), (1.0,)), ('EXP_BOUNDED', (-0.0,), (1.0,)), ('EXP_BOUNDED', (1e6,), (INF,)),
    ('EXP_BOUNDED', (-1e6,), (0.0,)), ('EXP_BOUNDED', (INF,), (NAN,)), ('EXP_BOUNDED', (-INF,), (NAN,)), ('EXP_BOUNDED', (NAN,), (NAN,)),
    ('EXP_SMALL', (0.0,), (1.0,)), ('EXP_SMALL', (-0.0,), (1.0,)), ('EXP_SMALL', (NAN,), (NAN,)),
    ('CEXP', (0.0, 0.0), (1.0, 0.0)), ('CEXP', (-INF, 0.0), (0.0, 0.0)), ('CEXP', (800.0, 0.0), (INF, NAN)),
    ('CEXP', (0.0, INF), (NAN, NAN)), ('CEXP', (NAN, 0.0), (NAN, NAN)), ('CEXP', (0.0, 1e12), (NAN, NAN)),
    ('CEXP_BOUNDED', (0.0, 0.0), (1.0, 0.0)), ('CEXP_BOUNDED', (1e6, 0.0), (INF, NAN)), ('CEXP_BOUNDED', (-1e6, 1.0), (0.0, 0.0)),
    ('CEXP_BOUNDED', (-INF, 0.0), (NAN, NAN)), ('CEXP_BOUNDED', (0.0, INF), (NAN, NAN)),
    ('CEXP_PAIR', (0.0, 0.0, 1e6, 0.0), (1.0, 0.0, INF, NAN)), ('CEXP_PAIR', (NAN, 0.0, 0.0, 0.0), (NAN, NAN, 1.0, 0.0)),
    ('CEXP_PAIR', (-1e6, 1.0, 0.0, INF), (0.0, 0.0, NAN, NAN)),
    ('FRCP', (0.0,), (INF,)), ('FRCP', (-0.0,), (-INF,)), ('FRCP', (INF,), (0.0,)), ('FRCP', (-INF,), (-0.0,)), ('FRCP', (NAN,), (NAN,)),
    ('FSQRT', (0.0,), (0.0,)), ('FSQRT', (-0.0,), (-0.0,)), ('FSQRT', (INF,), (INF,)), ('FSQRT', (-1.0,), (NAN,)), ('FSQRT', (NAN,), (NAN,)),
    ('FSQRT_HINV', (0.0,), (0.0, INF)), ('FSQRT_HINV', (INF,), (INF, 0.0)), ('FSQRT_HINV', (-1.0,), (NAN, NAN)),
    ('FSQRT_HINV', (NAN,), (NAN, NAN)),
    ('CRECIP', (0.0, 0.0), (NAN, NAN)), ('CRECIP', (2.0, 0.0), (0.5, -0.0)),
    ('CSQRT_FAST', (0.0, 0.0), (NAN, 0.0)), ('CSQRT_FAST', (4.0, 0.0), (2.0, 0.0)), ('CSQRT_FAST', (-4.0, 0.0), (0.0, 2.0)),
    ('CSQRT_FAST', (-4.0, -0.0), (0.0, -2.0)),
    ('CSQRT', (0.0, 0.0), (0.0, 0.0)), ('CSQRT', (-4.0, 0.0), (0.0, 2.0)), ('CSQRT', (-4.0, -0.0), (0.0, -2.0)),
    ('CSQRT', (0.0, 2.0), (1.0, 1.0)), ('CSQRT', (NAN, 1.0), (NAN, NAN)),
    ('CDIV', (1.0, 1.0, 0.0, 0.0), (NAN, NAN)), ('CDIV', (1.0, 1.0, 1.0, 1.0), (1.0, 0.0)),
    ('CMUL', (INF, 0.0, 0.0, 1.0), (NAN, INF)), ('CMUL', (NAN, 1.0, 1.0, 1.0), (NAN, NAN)), ('CMUL', (1.0, 2.0, 3.0, 4.0), (-5.0, 10.0)),
    ('CMADD', (1.0, 1.0, 1.0, 2.0, 3.0, 4.0), (-4.0, 11.0)), ('CMADD', (INF, 0.0, -INF, 0.0, 1.0, 0.0), (NAN, NAN)),
    ('CMSUB', (1.0, 1.0, 1.0, 2.0, 3.0, 4.0), (6.0, -9.0)), ('CMSUB', (0.0, NAN, 1.0, 0.0, 1.0, 0.0), (-1.0, NAN)),
    ('NEGATE_IF2', (NAN, 2.0), (NAN,)), ('NEGATE_IF2', (0.0, 2.0), (-0.0,)), ('NEGATE_IF2', (-INF, 2.0), (INF,)),
    ('NEGATE_IF2', (-0.0, 0.0), (-0.0,)),
    ('SIGNS_DIFFER', (NAN, -NAN), (1.0,)), ('SIGNS_DIFFER', (0.0, -0.0), (1.0,)), ('SIGNS_DIFFER', (-INF, -1.0), (0.0,)),
    ('SIGNS_DIFFER', (NAN, 1.0), (0.0,)),
    ('SCAN_CELL', (NAN, 3.0), (NAN, NAN)), ('SCAN_CELL', (INF, 3.0), (INF, INF)),
]


def test_special_values():
    for op, args, want in SPECIAL:
        with np.errstate(all='ignore'):
            got = host(op, *[np.array([a]) for a in args])[0]
        assert same_bits(got, np.array(want)), (op, args, got, want)            # the signs of zeros included
    s, c = host('SINCOS', mc.SINCOS_SPECIAL).T
    assert np.isfinite(s[:12]).sum() == 11 and np.isnan(s[10]) and np.isnan(s[12:]).all() and same_bits(np.isnan(s), np.isnan(c))


def test_no_nan_inside_the_domains():
    """Finite arguments inside each op's stated domain: every op returns, and nothing is NaN."""
    pos = mc.scaled_set(300, n=20000)
    re_, im = (v[:20000] for v in mc.csqrt_fast_set())
    sets = dict(SINCOS=(np.concatenate([s[1][:5000] for s in mc.sincos_segments()]),),
                EXP=(np.concatenate((mc.exp_segments(20000)[1][1], mc.exp_subnormal_set(5000), [-1e300, 1e300])),),
                EXP_BOUNDED=(np.concatenate((mc.exp_segments(20000)[1][1], [-1e6, 1e6])),), EXP_SMALL=(mc.exp_small_set(),),
                CEXP=mc.cexp_segments(20000)[1][1:], CEXP_BOUNDED=mc.cexp_segments(20000)[1][1:],
                FRCP=(mc.scaled_set(300, n=20000, signed=True),), FSQRT=(pos,), FSQRT_HINV=(pos,),
                CRECIP=(re_, im), CSQRT_FAST=(re_, im), CSQRT=(re_, im), CDIV=tuple(v[:20000] for v in mc.cdiv_set()),
                CMUL=tuple(v[:20000] for v in mc.fma_chain_set(4)), CMADD=tuple(v[:20000] for v in mc.fma_chain_set(6)),
                CMSUB=tuple(v[:20000] for v in mc.fma_chain_set(6)), SIGNS_DIFFER=(mc.bit_pattern_set(20000)[:20000], pos),
                SCAN_CELL=(pos, np.arange(20000) % 64))
    ra, ia, rb, ib, kind = mc.cexp_pair_waves(256)
    keep = ~(np.isnan(ra) | np.isnan(rb))
    sets['CEXP_PAIR'] = (ra[keep], ia[keep], rb[keep], ib[keep])
    b = mc.bit_pattern_set(20000)
    sets['NEGATE_IF2'] = (b[~np.isnan(b)], 2.0 * (np.arange((~np.isnan(b)).sum()) % 2))
    assert set(sets) == set(mc.OP_NAMES)
    for op, cols in sets.items():
        assert len(cols) == mc.N_IN[op], op
        with np.errstate(all='ignore'):
            assert not np.isnan(host(op, *cols)).any(), op


def test_host_forms_of_the_bit_tricks():
    """bh_negate_if2 against -x, bh_signs_differ against the sign bits, swd_scan_cell against the repeated addition,
    rf_cexp_pair against cexp_bounded of each argument, the short exponential against the full form: the host sides of
    what the GPU tier compares with the device."""
    x = mc.bit_pattern_set(1 << 17)
    two = 2.0 * (np.arange(x.size) % 2)
    got = host('NEGATE_IF2', x, two)[:, 0]
    want = np.where(two != 0, -x, x)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))               # NaN payloads too
    y = mc.bit_pattern_set(1 << 17, seed=13)
    assert np.array_equal(host('SIGNS_DIFFER', x, y)[:, 0], (np.signbit(x) != np.signbit(y)).astype(np.float64))
    base, cell, b, cn = mc.scan_cell_set()
    assert same_bits(host('SCAN_CELL', base, cell), np.stack((b, cn), axis=1))
    ra, ia, rb, ib, kind = mc.cexp_pair_waves(1024)
    pair = host('CEXP_PAIR', ra, ia, rb, ib)
    assert same_bits(pair[:, :2], host('CEXP_BOUNDED', ra, ia)) and same_bits(pair[:, 2:], host('CEXP_BOUNDED', rb, ib))
    xs = mc.exp_small_set()
    assert np.array_equal(host('EXP_SMALL', xs).view(np.int64), host('EXP_BOUNDED', xs).view(np.int64))


def test_selftest_math_validates_its_arguments(lib):
    """bh_selftest_math refuses an unknown op, a negative n and null pointers before any device work."""
    from bayhunter_amd import _lib
    a, out = np.zeros((4, mc.MP_IN)), np.zeros((4, mc.MP_OUT))
    for op, n, pin, pout in ((-1, 4, a.ctypes.data, out.ctypes.data), (len(mc.OP_NAMES), 4, a.ctypes.data, out.ctypes.data),
                             (0, -1, a.ctypes.data, out.ctypes.data), (0, 4, None, out.ctypes.data), (0, 4, a.ctypes.data, None)):
        assert lib.bh_selftest_math(op, n, pin, pout) == _lib.BH_ERR_ARG, (op, n)
    import bayhunter_amd as bh
    if bh.device_count() == 0:
        assert lib.bh_selftest_math(0, 4, a.ctypes.data, out.ctypes.data) == _lib.BH_ERR_NO_DEVICE
