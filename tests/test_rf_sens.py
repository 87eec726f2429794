"""Receiver-function sensitivity kernels on the CPU: the host twin of rf_sens_kernel (tests/hostsim/rf_sens_sim.cpp:
rf_sens_core.h built with g++ and the device math) against

* the independent longdouble reference (tests/rf_sens_ref.py: central differences of hp_oracle.rf_model_ld at two steps,
  Richardson) over rf_sens_cases.CASES within tests/rf_sens_tolerances.py, and off that list within the bounds there;
* the identity density scaling gives any exact trace: sum_i rho_i K_rho,i(t) = 0;
* the edge cases: nlay = 1 and nlay = Lmax, a zero entry, the half-space's K_h, nlay out of range;
* the argument checks of the C ABI, without a device, and of the Python entry points;
* itself under AddressSanitizer and UBSan, as a stand-alone program.
(What needs the device is in test_gpu_rf_sens.py.)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rf_sens_cases as rc
import rf_sens_ref
import rf_sens_tolerances as tol
from conftest import ROOT

KINDS = tol.KINDS
TUNED = [c for c in rc.CASES if c[0] != 'L1']


@pytest.fixture(scope='module')
def twin():
    return rc.load_sim()


def _ids(c):
    return '%s-%s-%d' % c


# ---- twin against the reference ---------------------------------------------------------------------------------------------
def test_the_reference_alone_stays_inside_its_cap_on_both_lists():
    for keys in (TUNED, list(rc.OFFLIST)):
        flagged, total = rc.reference_flags(keys)
        print('flagged %d of %d' % (flagged, total))
        assert flagged <= rf_sens_ref.CAP * total


@pytest.mark.parametrize('case', TUNED, ids=_ids)
def test_twin_against_the_longdouble_reference(twin, case):
    name, ref, nsamp = case
    par = rc.params(ref, nsamp)
    K, rf = twin.row(*rc.MODELS[name], par)
    R = rc.references([case])[case]
    err, own, left_out = tol.errors(K, R)
    print('%s: ' % (case,) + ', '.join('%s %.2e (%.2e; reference %.2e)' % (k, err[k], tol.tolerance(k), own[k]) for k in KINDS))
    assert left_out <= rf_sens_ref.CAP * K.shape[0] * (4 * K.shape[2] - 1)
    for k in KINDS:
        assert err[k] <= tol.tolerance(k), (k, err[k], tol.tolerance(k))
        assert own[k] <= tol.REFERENCE_OWN[k] * 1.005, (k, own[k])                 # the recorded estimates hold
    assert np.isfinite(K).all() and np.all(K[:, 0, -1] == 0)                       # the half-space has no thickness
    assert all(np.abs(K[:, k]).max() > 0 for k in range(4))
    scale = max(1.0, np.abs(rf).max())
    assert np.abs(rf - R['rf'].astype(np.float64)).max() <= 1e-10 * scale          # the trace itself (tolerances.TOL_RF)


@pytest.mark.parametrize('name', list(rc.OFFLIST))
def test_twin_against_the_reference_off_the_list(twin, name):
    """Nothing was tuned on these models: the error is below the bound recorded next to its measured value."""
    worst, _ = tol.measure(twin, [name])
    print('%s: ' % name + ', '.join('%s %.2e (%.2e)' % (k, v, tol.offlist_bound(k)) for k, v in worst.items()))
    for k, v in worst.items():
        assert np.isfinite(v) and v <= tol.offlist_bound(k), (k, v)


def test_the_recorded_steps_are_the_librarys_and_the_tolerances_follow_the_measurements(twin):
    src = open(os.path.join(ROOT, 'bayhunter_amd', 'csrc', 'rf_sens_core.h')).read()
    assert 's.h = 0x1p%d; s.vp = 0x1p%d; s.vs = 0x1p%d; s.rho = 0x1p%d;' % tuple(tol.STEPS_LOG2[k] for k in KINDS) in src
    assert np.array_equal(twin.steps(), [2.0 ** tol.STEPS_LOG2[k] for k in KINDS])
    for k in KINDS:
        assert tol.SWEEP[k][tol.SWEEP_LOG2.index(tol.STEPS_LOG2[k])] == tol.MEASURED[k] == min(tol.SWEEP[k])
        assert tol.tolerance(k) == 2.0 * tol.MEASURED[k] and tol.offlist_bound(k) == 2.0 * tol.OFFLIST_MEASURED[k]
        assert 4.0 * tol.REFERENCE_OWN[k] <= tol.MEASURED[k]


def test_a_swept_step_moves_the_error_as_recorded(twin):
    """Two lines of the sweep again: the thickness step at 2^-21 and the vs step at 2^-15, over the whole list."""
    for kind, p in (('h', -21), ('vs', -15)):
        steps = [2.0 ** (p if k == kind else tol.STEPS_LOG2[k]) for k in KINDS]
        worst, _ = tol.measure(twin, TUNED, steps=steps)
        rec = tol.SWEEP[kind][tol.SWEEP_LOG2.index(p)]
        assert 2 * tol.MEASURED[kind] < worst[kind] <= rec * 1.005, (kind, p, worst[kind])


# ---- identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TUNED, ids=_ids)
def test_density_scaling_identity(twin, case):
    name, ref, nsamp = case
    K, _ = twin.row(*rc.MODELS[name], rc.params(ref, nsamp))
    res = tol.identity_residual(K, rc.MODELS[name][3])
    print(case, 'residual %.2e (%.2e)' % (res, tol.identity_tolerance()))
    assert res <= tol.identity_tolerance()


# ---- edge cases -------------------------------------------------------------------------------------------------------------
def test_edge_cases(twin):
    par = rc.params('prf', 64, nout=40)
    m = rc.MODELS['L3']
    K, rf = twin.row(*m, par)                                                      # nlay = Lmax
    assert K.shape == (40, 4, 3) and np.isfinite(K).all() and np.all(K[:, 0, 2] == 0) and np.isfinite(rf).all()
    Kp, rfp = twin.row(*m, par, nlay=3, Lmax=7)                                    # padded: the same values, NaN behind
    assert np.array_equal(Kp[:, :, :3], K) and np.isnan(Kp[:, :, 3:]).all() and np.array_equal(rfp, rf)
    # a zero entry has no relative step: 0, and nothing else moves (the half-space's thickness entry is not read)
    h0 = m[0].copy()
    h0[2] = 5.0
    K0, _ = twin.row(h0, *m[1:], par)
    assert np.array_equal(K0, K)
    rho0 = m[3].copy()
    rho0[1] = 0.0
    Kz, _ = twin.row(m[0], m[1], m[2], rho0, par)
    assert np.all(Kz[:, 3, 1] == 0)
    # a half-space alone: the spectral division is 0 / 0 -- NaN trace and kernels, in the reference too; K_h stays 0
    for ref in ('prf', 'srf'):
        p1 = rc.params(ref, 128)
        K1, rf1 = twin.row(*rc.MODELS['L1'], p1)
        R1 = rf_sens_ref.kernels(*rc.MODELS['L1'], p1)
        assert np.isnan(rf1).all() and np.isnan(R1['rf'].astype(np.float64)).all()
        assert np.all(K1[:, 0, 0] == 0) and np.isnan(K1[:, 1:, 0]).all() and np.isnan(R1['K'][:, 1:, 0].astype(np.float64)).all()
    # nlay out of range: NaN throughout
    for bad in (0, -3, 8):
        Kb, rfb = twin.row(*m, par, nlay=bad, Lmax=7)
        assert np.isnan(Kb).all() and np.isnan(rfb).all()
    # the slot numbering covers every entry but the half-space's thickness once
    for n in (1, 2, 7):
        seen = sorted(twin.lib.rs_slot(n, s) for s in range(4 * n - 1))
        assert seen == sorted(k * 1000 + i for k in range(4) for i in range(n) if not (k == 0 and i == n - 1))


# ---- without a device -------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_before_it_touches_a_device(lib):
    from bayhunter_amd import _lib
    p = C.c_void_p(64)            # never dereferenced: every call below is refused first

    def batch(B=4, Lmax=8, mstride=8, null=None, k_stride=None, rf=True, rf_stride=None, **par):
        d = dict(p=6.4, gauss=1.0, fsamp=5.0, tshift=5.0, nsv=-1.0, nsamp=64, waveno=0, nout=40, out_off=0)
        d.update(par)
        c = _lib.RfParams(d['p'], d['gauss'], d['fsamp'], d['tshift'], d['nsv'], d['nsamp'], d['waveno'], d['nout'], d['out_off'])
        a = [B, Lmax, mstride, p, p, p, p, p, None, None, C.byref(c), p, d['nout'] * 4 * Lmax if k_stride is None else k_stride,
             p if rf else None, d['nout'] if rf_stride is None else rf_stride, None, 0, None]
        if null is not None:
            a[null] = None
        return lib.bh_rf_sens_batch(*a)

    for kw, msg in ((dict(null=10), b'par is NULL'), (dict(B=-1), b'B/Lmax'), (dict(Lmax=0), b'B/Lmax'),
                    (dict(Lmax=_lib.MAX_LAYERS + 1, mstride=200), b'B/Lmax'), (dict(mstride=7), b'model_stride < Lmax'),
                    (dict(nsamp=48), b'power of two'), (dict(nsamp=4), b'power of two'), (dict(nsamp=8192), b'power of two'),
                    (dict(waveno=2), b'waveno'), (dict(nout=0), b'nout out of range'), (dict(nout=65), b'nout out of range'),
                    (dict(gauss=0.0), b'gauss and fsamp'), (dict(fsamp=-1.0), b'gauss and fsamp'),
                    (dict(k_stride=40 * 4 * 8 - 1), b'k_stride shorter'), (dict(rf_stride=39), b'rf_stride shorter')) \
            + tuple((dict(null=i), b'NULL pointer') for i in (3, 4, 5, 6, 7, 11)):
        assert batch(**kw) == _lib.BH_ERR_ARG, kw
        assert msg in lib.bh_last_error(), (kw, lib.bh_last_error())
    # 2^31 - 1 models of 100 layers are more workgroups than a launch has
    assert batch(B=0x7fffffff, Lmax=100, mstride=100) == _lib.BH_ERR_ARG and b'do not fit one launch' in lib.bh_last_error()
    assert batch(B=0) == _lib.BH_OK and batch(B=0, rf=False) == _lib.BH_OK
    assert batch(B=0, out_off=1000) == _lib.BH_OK                                   # out_off is ignored
    assert lib.bh_rf_sens_workspace_bytes(10, 256) == 0
    z = np.zeros(4)
    K, x = np.zeros(64 * 4 * 4), np.zeros(64)

    def single(nsamp=64, n=4, null=None, fz=None, fr=None):
        a = [nsamp, 5.0, 5.0, 6.4, 1.0, -1.0, float('nan'), 0, n] + [z.ctypes.data] * 6 + [fz, fr, x.ctypes.data, K.ctypes.data]
        if null is not None:
            a[null] = None
        return lib.bh_rf_sensitivity(*a)
    for kw in (dict(null=18), dict(null=17), dict(null=9), dict(null=12), dict(null=14), dict(n=0), dict(n=101), dict(nsamp=4),
               dict(nsamp=8192), dict(fz=x.ctypes.data)):
        assert single(**kw) == _lib.BH_ERR_ARG, kw
        assert lib.bh_last_error()


def test_python_entry_points_check_their_arguments_before_a_device():
    from bayhunter_amd import plugins, sensitivity as S
    t = np.arange(40) / 5.0 - 5.0
    with pytest.raises(ValueError, match='rfparams'):
        S.rf_batch(dict(gauss=1.0), *[np.zeros((2, 3))] * 4, [3, 3])
    with pytest.raises(ValueError, match='rfparams'):
        S.rf_batch(dict(obsx=t, slowness=6.4), *[np.zeros((2, 3))] * 4, [3, 3])
    p = plugins.RFminiModRF(t, 'prf')
    with pytest.raises(AssertionError):
        p.sensitivity(np.zeros(3), np.zeros(3), np.zeros(2), np.zeros(3))
    p.set_modelparams(wtype='SH')
    with pytest.raises(ValueError, match='SH'):
        p.sensitivity(*rc.MODELS['L3'])


# ---- sanitizers -------------------------------------------------------------------------------------------------------------
def test_host_twin_under_asan_ubsan(tmp_path):
    """rf_sens_core.h and the twin's own code as a stand-alone program (RF_SENS_SIM_MAIN) under AddressSanitizer and
    UBSan."""
    exe = str(tmp_path / 'rf_sens_sim')
    c = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-omit-frame-pointer', '-DRF_SENS_SIM_MAIN', rc.SIM_SRCS[0], '-o', exe], capture_output=True, text=True)
    if c.returncode != 0 and ('cannot find' in c.stderr or 'sanitizer' in c.stderr.lower()):
        pytest.skip('sanitizer runtime not installed: ' + c.stderr[-300:])
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, UBSAN_OPTIONS='print_stacktrace=1'))
    if 'Shadow memory range interleaves' in r.stderr or 'ReserveShadowMemoryRange failed' in r.stderr:
        pytest.skip('the sanitizer runtime cannot start in this environment: ' + r.stderr[-300:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'rf sens ok' in r.stdout and 'runtime error' not in r.stderr, r.stderr[-4000:]
