"""GPU tier: the layer step's reused reciprocals (bh_common.h: xsqrt_recip_nz, recip_sq) leave every bit where it
was.

1. bh_selftest_division, whose kernel now also compares a / sqrt(x) through the root's by-product reciprocal,
   a / (b*b) through the squared reciprocal (b with a 24-bit mantissa) and the guard-free root itself against the
   IEEE operators: 0 mismatches at both exponent ranges of tests/test_gpu_parity.py::test_division_selftest.
2. Models that reach the branches random models never reach.  The guard-free root is NaN for a zero argument, which
   happens when the trial wavenumber equals a layer's (wvno == xka or wvno == xkb); the layer step must then take
   the branch that reads neither the root nor its reciprocal.  The first period's bracketing scan evaluates
   c = c0 + k dc (c0 = 0.855 x the half-space Rayleigh velocity of the slowest layer, an fp32 value; dc = 0.005f;
   the sums are exact in fp64), so a layer whose vs or vp is such a c that happens to be an fp32 value, below the
   first period's phase velocity, is met exactly.  Plus water-layer models (swd_var with the constant 1e-5 in place
   of rb).  All monotone, so the device must equal the oracle (port backend) bit for bit, on every kernel form.

_constructed() asserts that each special velocity lies on the grid above c0, and the test that it lies below the
oracle's first phase velocity, i.e. that the scan passes it.  Checked on the CPU when the cases were chosen: a
replay of swd_core.h with a counter in the three `==` branches took each case's branch exactly once (Rayleigh phase
and group: all 8; Love: the 5 vs cases), and the oracle finds a root for all of them (0 of 8 skipped; the limit is
a quarter).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER = np.linspace(25.0, 45.0, 6)
DC = float(np.float32(0.005))


def _gtsolh(a, b):
    """swd_gtsolh (surfdisp96.f:367-388) in the reference's real*4 arithmetic."""
    f = np.float32
    a, b = f(a), f(b)
    c = f(0.95) * b
    for _ in range(5):
        gamma, kappa = b / a, c / b
        k2 = kappa * kappa
        gk = gamma * kappa
        gk2 = gk * gk
        fac1, fac2 = np.sqrt(f(1.0) - gk2), np.sqrt(f(1.0) - k2)
        tk = f(2.0) - k2
        fr = tk * tk - f(4.0) * fac1 * fac2
        frp = (-f(4.0) * (f(2.0) - k2) * kappa + f(4.0) * fac2 * gamma * gamma * kappa / fac1
               + f(4.0) * fac1 * kappa / fac2)
        frp = frp / b
        c = c - fr / frp
    assert c.dtype == np.float32
    return c


def _scan_start(vp, vs):
    """c0 of the search (swd_driver: 0.90 * 0.95 * gtsolh of the slowest solid layer), solid models."""
    j = int(np.argmin(vs))
    c = _gtsolh(vp[j], vs[j])
    c = np.float32(0.95) * c
    c = np.float32(0.90) * c
    return float(c)


def _grid_value(c0, lo, hi):
    """The first c = c0 + dc + dc + ... (fp64, as the scan adds) in (lo, hi) that is an fp32 value, and its k."""
    c, k = c0, 0
    while c < hi:
        if c > lo and float(np.float32(c)) == c:
            return c, k
        c, k = c + DC, k + 1
    raise AssertionError('no fp32 value on the grid in (%g, %g)' % (lo, hi))


def _base(top_vs):
    vs = np.array([top_vs, 1.9, 2.6, 3.3, 3.9, 4.6])
    vp = np.array([top_vs * 1.9, 3.2, 4.5, 5.8, 6.8, 8.1])
    h = np.array([1.0, 2.5, 5.0, 9.0, 14.0, 0.0])
    return h, vp, vs


# (top layer's vs -> c0; which array and layer receives the grid value; the window it is looked for in)
CASES = [(1.00, 'vs', 1, 1.3, 2.5), (1.10, 'vs', 2, 2.0, 3.2), (0.90, 'vs', 2, 2.0, 3.2), (1.20, 'vs', 1, 1.4, 2.5),
         (1.05, 'vp', 1, 2.7, 3.45), (0.95, 'vp', 1, 2.7, 3.45), (1.15, 'vs', 2, 2.0, 3.2), (0.85, 'vp', 1, 2.7, 3.45)]


def _constructed():
    """[B, 6] models (fp32 values in fp64 arrays) and the special velocity of each."""
    H, VP, VS, CS = [], [], [], []
    for top, which, lay, lo, hi in CASES:
        h, vp, vs = _base(top)
        h, vp, vs = (x.astype(np.float32).astype(np.float64) for x in (h, vp, vs))
        c0 = _scan_start(vp, vs)
        c, k = _grid_value(c0, lo, hi)
        if which == 'vs':                                         # the layer's other velocity follows (vp / vs = 1.75)
            vs[lay], vp[lay] = c, float(np.float32(1.75 * c))
        else:
            vp[lay], vs[lay] = c, float(np.float32(c / 1.75))
        assert np.all(np.diff(vs) > 0) and np.all(vp > 1.5 * vs) and _scan_start(vp, vs) == c0 and k > 0
        H.append(h); VP.append(vp); VS.append(vs); CS.append(c)
    H, VP, VS = np.array(H), np.array(VP), np.array(VS)
    RHO = (VP * 0.32 + 0.77).astype(np.float32).astype(np.float64)
    return H, VP, VS, RHO, np.array(CS)


def _water():
    """The constructed models under 0.5 .. 4 km of water (vs = 0: llw = 2, the water-layer tail of dltar4)."""
    H, VP, VS, RHO, _ = _constructed()
    B = H.shape[0]
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    H = np.concatenate([f32(np.linspace(0.5, 4.0, B))[:, None], H], axis=1)
    VP = np.concatenate([f32(np.full((B, 1), 1.5)), VP], axis=1)
    VS = np.concatenate([np.zeros((B, 1)), VS], axis=1)
    RHO = np.concatenate([f32(np.full((B, 1), 1.03)), RHO], axis=1)
    return H, VP, VS, RHO


def test_division_selftest_covers_the_reused_reciprocals(lib):
    from bayhunter_amd import _lib
    for n, max_exp in ((1 << 26, 40), (1 << 24, 300)):
        bad = C.c_long(-1)
        _lib.check(lib.bh_selftest_division(n, 777 + max_exp, max_exp, C.byref(bad)))
        print('selftest max_exp %d: %d mismatches in %d samples' % (max_exp, bad.value, n))
        assert bad.value == 0, (max_exp, bad.value)


def _run_forms(specs, models, nl):
    from bayhunter_amd import _lib
    from bayhunter_amd.engine import ForwardEngine
    eng = ForwardEngine(swd=specs)
    got = {}
    for form in ('lane', 'team8', 'team', 'team128'):
        _lib.set_swd_kernel(form)
        try:
            out, err = eng.run(*models, nl)
            got[form] = (out.cpu().numpy(), err.cpu().numpy())
        finally:
            _lib.set_swd_kernel('auto')
    return eng, got


def test_trial_velocity_equal_to_a_layer_velocity(lib, oracle):
    from bayhunter_amd.engine import SwdSpec
    H, VP, VS, RHO, CS = _constructed()
    B = H.shape[0]
    nl = np.full(B, H.shape[1], dtype=np.int32)
    refs = [('rdispph', 2, 0), ('ldispph', 1, 0), ('rdispgr', 2, 1)]
    eng, got = _run_forms([SwdSpec(r[0], PER) for r in refs], (H, VP, VS, RHO), nl)
    for t, (name, iwave, igr) in enumerate(refs):
        want, werr, _ = oracle.swd_batch(H, VP, VS, RHO, nl, PER, iwave, igr)
        ok = werr == 0                                            # the oracle itself finds no root: not a case
        assert (~ok).sum() * 4 <= B, (name, werr)
        if igr == 0:
            # the scan of the first period goes up from c0 in steps of dc until it has passed the root: it evaluates
            # the special velocity exactly (Love only meets vs)
            hit = ok & (CS < want[:, 0])
            if iwave == 1:
                hit &= np.array([c[1] == 'vs' for c in CASES])
            print('%s: %d of %d cases pass their special velocity' % (name, hit.sum(), B))
            assert hit.sum() * 4 >= 3 * (B if iwave == 2 else sum(c[1] == 'vs' for c in CASES)), (name, CS, want[:, 0])
        for form, (out, err) in got.items():
            assert np.array_equal(err[:, t], werr), (name, form)
            o = out[:, eng.slices[t]]
            assert np.array_equal(o[ok].view(np.int64), want[ok].view(np.int64)), (name, form, o[ok] - want[ok])


def test_water_layer_models(lib, oracle):
    from bayhunter_amd.engine import SwdSpec
    H, VP, VS, RHO = _water()
    B = H.shape[0]
    nl = np.full(B, H.shape[1], dtype=np.int32)
    refs = [('rdispph', 2, 0), ('rdispgr', 2, 1)]
    eng, got = _run_forms([SwdSpec(r[0], PER) for r in refs], (H, VP, VS, RHO), nl)
    for t, (name, iwave, igr) in enumerate(refs):
        want, werr, _ = oracle.swd_batch(H, VP, VS, RHO, nl, PER, iwave, igr)
        ok = werr == 0
        assert (~ok).sum() * 4 <= B, (name, werr)
        for form, (out, err) in got.items():
            assert np.array_equal(err[:, t], werr), (name, form)
            o = out[:, eng.slices[t]]
            assert np.array_equal(o[ok].view(np.int64), want[ok].view(np.int64)), (name, form, o[ok] - want[ok])
