"""rf_kernel's attenuation exponent without range reduction (rf_core.h: rf_exp_small, taken when a wave-uniform test
finds every active lane inside |x| <= 0.34) and the radix-4 passes of its inverse transform (rf_fft_butterfly4), on the
CPU: the host replay of rf_host.h -- the phase functions, the transform's plan and the butterflies the kernel runs --
against the oracle, which computes every frequency bin with glibc's exp and a radix-2 transform.

Both changes are exact by construction, and the first tests say so: inside its bound the short exponential returns the
bits of the full form (k = 0 in the reduction, ldexp by 0), and a radix-4 pass forms the products and sums of the two
radix-2 stages it replaces in the same order.  The host replay therefore equals the parent's replay (every stage
radix-2, every exponential reduced) bit for bit, and the deviation from the oracle is the parent's:

    worst |replay - oracle| / max(1, |oracle|)        parent (52e133e)    this code
    rf_extreme.resonant_models(400) (Q_s 5 ... 225)   3.181e-15           same
    2 000 bench-seed models (draw_models, seed 1)     3.626e-16           same
    mixed_bound_models(40) (Q_s = 5, 10-15 km slow)   1.388e-16           same

(tests/rf_extreme.py's model set and the resonant low-Q set of test_rf_lean.py are the same draw, resonant_models(400)
with its default seed.)  The assertions: the project's tolerance TOL_RF, and no more than twice the parent's figure of
the set -- the factor is there so that a real loss of accuracy shows while a reordering of roundings would not; the
parent's figures differ by a factor of ten between the sets, so it is applied set by set.  Each test prints its figure
before it asserts."""
import numpy as np
import pytest

from bayhunter_amd.synthetic import draw_models
from rf_extreme import resonant_models
from rf_floor_cases import GAUSS_ALL, attenuation_exponents, floor_sim, mixed_bound_models, replay
from tolerances import TOL_RF

# measured with the parent's host replay (hostsim.cpp: hs_rf, device math) on the same inputs, profiles/r12_ab_rf_floor.txt
PARENT = dict(extreme=3.181e-15, draw=3.626e-16, mixed=1.388e-16)
N_EXTREME, N_DRAW, N_MIXED = 400, 2000, 40


def _ptr(a):
    return a.ctypes.data


def test_short_exponential_is_the_full_form_bit_for_bit():
    hs = floor_sim()
    rs = np.random.RandomState(3)
    b = 0.34
    x = np.concatenate(([0.0, -0.0, b, -b, np.nextafter(b, 0), -np.nextafter(b, 0), 5e-324, -5e-324, 1e-300, 1e-17],
                        rs.uniform(-b, b, 200000), rs.uniform(-1e-3, 1e-3, 20000), np.linspace(-b, b, 20001)))
    small, full = np.zeros_like(x), np.zeros_like(x)
    assert hs.hs_exp_forms(x.size, _ptr(x), _ptr(small), _ptr(full)) == b       # the bound the kernel tests
    assert b < 0.5 * np.log(2.0)                                             # k = rint(x log2 e) = 0 inside it
    assert np.array_equal(small.view(np.int64), full.view(np.int64))
    exact = np.exp(x.astype(np.longdouble))                                  # (64-bit mantissa: 2^-11 ulp of a double)
    ulp = (np.abs(small.astype(np.longdouble) - exact) / np.spacing(small)).astype(np.float64)
    print('rf_floor: short exponential against exp in extended precision, worst %.3f ulp over %d arguments' % (ulp.max(), x.size))
    assert ulp.max() < 1.0


def test_phase_factors_do_not_depend_on_the_form_taken():
    """rf_cexp_pair, the pair of phase factors of a layer: both arguments inside the bound (short form), one outside,
    both outside, NaN -- always the bits of cexp_bounded of each argument."""
    hs = floor_sim()
    rs = np.random.RandomState(4)
    n = 60000
    re_a = np.where(rs.rand(n) < 0.5, rs.uniform(-0.34, 0.34, n), rs.uniform(-12.0, 1.0, n))
    re_b = np.where(rs.rand(n) < 0.5, rs.uniform(-0.34, 0.34, n), rs.uniform(-12.0, 1.0, n))
    re_a[:4] = [np.nan, 0.1, -800.0, 0.34]
    re_b[:4] = [0.1, np.nan, 0.2, -0.34]
    za = np.ascontiguousarray(np.stack((re_a, rs.uniform(-300.0, 300.0, n)), axis=1))
    zb = np.ascontiguousarray(np.stack((re_b, rs.uniform(-300.0, 300.0, n)), axis=1))
    pair, fa, fb = np.zeros((n, 4)), np.zeros((n, 2)), np.zeros((n, 2))
    hs.hs_cexp_pair(n, _ptr(za), _ptr(zb), _ptr(pair))
    hs.hs_cexp_full(n, _ptr(za), _ptr(fa))
    hs.hs_cexp_full(n, _ptr(zb), _ptr(fb))
    inside = (np.abs(re_a) <= 0.34) & (np.abs(re_b) <= 0.34)
    assert 0.15 * n < inside.sum() < 0.35 * n
    assert np.array_equal(pair[:, :2], fa, equal_nan=True) and np.array_equal(pair[:, 2:], fb, equal_nan=True)


@pytest.mark.parametrize('nsamp', [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024])
def test_radix4_passes_equal_the_radix2_stages(nsamp, hostsim_devmath):
    """log2 n odd (128, 512: one radix-2 stage first) and even (256, 1024): the transform in radix-4 passes, the same
    with every stage radix-2, and hostsim.cpp's replay, which drives the radix-2 butterflies itself: one trace."""
    H, VP, VS, RHO, nl = draw_models(3, (3, 10), seed=nsamp)
    for b in range(3):
        n = nl[b]
        nout = min(201, nsamp)
        kw = dict(p=6.4, gauss=1.0 if b else 2.0, nsamp=nsamp, fsamp=5.0, tshift=min(5.0, nsamp / 25.0), waveno=b & 1, nout=nout)
        r4 = replay(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n], radix4=True, **kw)
        r2 = replay(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n], radix4=False, **kw)
        old = hostsim_devmath.rf(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n], **kw)
        assert np.isfinite(r4).all() and np.abs(r4).max() > 0
        assert np.array_equal(r4, r2) and np.array_equal(r4, old)


def _bounded(tag, worst):
    print('rf_floor host replay, %s: worst %.3e (parent %.3e, tolerance %.1e)' % (tag, worst, PARENT[tag], TOL_RF))
    assert worst <= TOL_RF and worst <= 2.0 * PARENT[tag], (tag, worst, PARENT[tag])


def _worst_of(oracle, models, nsamp=512):
    worst, finite = 0.0, 0
    for m in models:
        want = oracle.synrf(m['z'], m['vp'], m['vs'], m['rho'], m['qp'], m['qs'], m['p'], m['gauss'], nsamp, 5.0, 5.0,
                            m['vs'][0], m['sigma'], m['waveno'])[2]
        got = replay(m['h'], m['vp'], m['vs'], m['rho'], m['p'], m['gauss'], nsamp, 5.0, 5.0, None, m['waveno'], nsamp,
                     qp=m['qp'], qs=m['qs'])
        assert np.array_equal(np.isfinite(want), np.isfinite(got))
        if np.isfinite(want).all():
            finite += 1
            worst = max(worst, np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    return worst, finite


def test_host_replay_rf_extreme(oracle):
    worst, finite = _worst_of(oracle, resonant_models(N_EXTREME))
    assert finite >= 300
    _bounded('extreme', worst)


def test_host_replay_bench_models():
    H, VP, VS, RHO, nl = draw_models(N_DRAW, 10, seed=1)
    from oracle import pyoracle
    want = pyoracle.rf_batch(H, VP, VS, RHO, nl, nthreads=8)
    worst = 0.0
    for b in range(N_DRAW):
        n = nl[b]
        got = replay(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n], 6.4, 1.0, 512, 5.0, 5.0, None, 0, want.shape[1])
        worst = max(worst, np.abs(got - want[b]).max() / max(1.0, np.abs(want[b]).max()))
    _bounded('draw', worst)


def test_mixed_bound_models_hold_both_forms_in_one_wave():
    """What the set is built for: among the first 64 frequencies of a model (its first wave of phase 3) there are steps
    well inside the bound and steps well outside it, and w reaches 15.7 rad/s."""
    for m in mixed_bound_models(N_MIXED):
        x = np.abs(attenuation_exponents(m)).max(axis=(1, 2))
        assert x.shape == (257,) and x[:64].min() < 0.3 and x[:64].max() > 0.4 and x[64:].min() > 0.4, x[[0, 1, 63, 64, 256]]
        assert 4.0 < x[256] < 12.0


def test_host_replay_mixed_bound_models(oracle):
    worst, finite = _worst_of(oracle, mixed_bound_models(N_MIXED))
    assert finite == N_MIXED and GAUSS_ALL >= 1.21
    _bounded('mixed', worst)
