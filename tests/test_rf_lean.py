"""The receiver-function recursion with its products written as multiply-add chains, the phase factors and the
reciprocal determinant merged into two row factors (rf_core.h: rf_layer_step), a select-free |z| in the complex
root and one LDS record per layer: deviation from the oracle, which computes every frequency bin, on the models
built to break the kernel (tests/rf_extreme.py) and on 2 000 random ten-layer models (what bench.py draws).

Each tier prints its worst deviation before it asserts.  The same tests run on the parent commit (14705aa,
whose recursion and layout were the old ones) gave, on the same inputs:

    tier                          rf_extreme (resonant, low Q)      2 000 draw_models
    host replay (device math)     3.279e-15 (this code 3.181e-15)   3.331e-16 (3.626e-16)
    MI355X (C ABI)                3.140e-15 (this code 3.258e-15)   5.274e-16 (5.274e-16)

The assertions are the project's tolerance for the class (tolerances.TOL_RF, relative to the trace's scale), not
those figures.  The bounded-exponent exponential and the radix-4 inverse FFT of the issue were not built, so there
is no exponent bound and no new transform to check here (test_hostsim.py::test_rf_every_transform_length and the
GPU tier's corner cases keep covering every nsamp with the radix-2 transform)."""
import numpy as np
import pytest

from bayhunter_amd.synthetic import draw_models
from rf_extreme import resonant_models
from tolerances import TOL_RF

N_EXTREME, N_DRAW = 400, 2000


def _worst_extreme(oracle, rf_of_model):
    worst, finite = 0.0, 0
    for m in resonant_models(N_EXTREME):
        want = oracle.synrf(m['z'], m['vp'], m['vs'], m['rho'], m['qp'], m['qs'], m['p'], m['gauss'], 512, 5.0, 5.0,
                            m['vs'][0], m['sigma'], m['waveno'])[2]
        got = rf_of_model(m)
        assert np.array_equal(np.isfinite(want), np.isfinite(got))
        if np.isfinite(want).all():
            finite += 1
            worst = max(worst, np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    return worst, finite


def _draw():
    H, VP, VS, RHO, nl = draw_models(N_DRAW, 10, seed=1)
    from oracle import pyoracle
    return (H, VP, VS, RHO, nl), pyoracle.rf_batch(H, VP, VS, RHO, nl, nthreads=8)


def test_host_replay_rf_extreme(oracle, hostsim_devmath):
    hs = hostsim_devmath
    worst, finite = _worst_extreme(oracle, lambda m: hs.rf(m['h'], m['vp'], m['vs'], m['rho'], m['p'], m['gauss'], 512,
                                                           5.0, 5.0, None, m['waveno'], 512, qp=m['qp'], qs=m['qs']))
    print('rf_lean host replay, rf_extreme: worst %.3e over %d finite models' % (worst, finite))
    assert finite >= 300 and worst <= TOL_RF, (finite, worst)


def test_host_replay_draw_models(hostsim_devmath):
    (H, VP, VS, RHO, nl), want = _draw()
    worst = 0.0
    for b in range(N_DRAW):
        n = nl[b]
        # the bench set-up: a = 1, p = 6.4 s/deg, 512 samples at 5 Hz shifted by 5 s, 201 samples returned
        got = hostsim_devmath.rf(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n], 6.4, 1.0, 512, 5.0, 5.0, None, 0,
                                 want.shape[1])
        worst = max(worst, np.abs(got - want[b]).max() / max(1.0, np.abs(want[b]).max()))
    print('rf_lean host replay, draw_models: worst %.3e over %d models' % (worst, N_DRAW))
    assert worst <= TOL_RF, worst


@pytest.mark.gpu
def test_gpu_rf_extreme(lib, oracle):
    from bayhunter_amd import _lib

    def synrf(m):
        a = [np.ascontiguousarray(m[k]) for k in ('z', 'vp', 'vs', 'rho', 'qp', 'qs')]
        rf = np.zeros(512)
        _lib.check(lib.bh_synrf(512, 5.0, 5.0, m['p'], m['gauss'], m['vs'][0], m['sigma'], m['waveno'], a[0].size,
                                *[x.ctypes.data for x in a], None, None, rf.ctypes.data))
        return rf
    worst, finite = _worst_extreme(oracle, synrf)
    print('rf_lean MI355X, rf_extreme: worst %.3e over %d finite models' % (worst, finite))
    assert finite >= 300 and worst <= TOL_RF, (finite, worst)


@pytest.mark.gpu
def test_gpu_draw_models(lib):
    from bayhunter_amd.engine import ForwardEngine, RfSpec
    (H, VP, VS, RHO, nl), want = _draw()
    eng = ForwardEngine(rf=[RfSpec('prf', np.linspace(-5, 35, 201))])
    assert int(lib.bh_rf_active_frequencies(eng._rfp[0])) == 213        # the Gauss cut-off stays at 3e-19
    out, err = eng.run(H, VP, VS, RHO, nl)
    got = out.cpu().numpy()
    scale = np.maximum(1.0, np.abs(want).max(axis=1))
    worst = float((np.abs(got - want).max(axis=1) / scale).max())
    print('rf_lean MI355X, draw_models: worst %.3e over %d models' % (worst, N_DRAW))
    assert worst <= TOL_RF, worst
