"""Group-velocity sensitivity kernels on the CPU: the host twin of sens_group_root_kernel / sens_group_kernel
(tests/hostsim/sens_group_sim.cpp: sens_group_core.h built with g++ and the device math) against

* the independent longdouble reference (tests/sens_group_ref.py: no Rodi formula -- U of every perturbed model from its
  own roots at neighbouring periods, then differenced over the parameter) over sensitivity_cases.CASES, within
  tests/sens_group_tolerances.py: K^U, U, dU/dT;
* the identities dimensional scaling gives any exact U(T, h, vp, vs, rho);
* sensitivity.group_velocity and the phase twin, bit for bit: U, c, K_phase;
* the rows without a value, a rejected side root, the zeros, and the argument checks of the C ABI and of the plugin;
* itself under AddressSanitizer and UBSan, as a stand-alone program.
(What needs the device is in test_gpu_sens_group.py.)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sens_group_cases as gc
import sens_group_ref as gref
import sens_group_tolerances as tol
import sensitivity_cases as sc
import sensitivity_ref as ref
from conftest import ROOT

KINDS = ('h', 'vp', 'vs', 'rho')
WHAT = ('U', 'dU_dT') + KINDS
OUT_KEYS = ('K', 'U', 'dU_dT', 'c', 'K_phase')


@pytest.fixture(scope='module')
def twin():
    return gc.load_sim()


_RESULTS = {}


def _case(twin, name, wave):
    """Twin and reference of one case, computed once and not changed: (model as real*4 values, twin dict, list of the
    reference's dicts per period)."""
    if (name, wave) not in _RESULTS:
        m = sc.MODELS[name]
        t = twin.sensitivity(*m, sc.PERIODS, wave)
        assert t['err'] == 0 and np.all(t['c0'] > 0)
        R = [gref.kernels(*m, T, c0, wave) for T, c0 in zip(sc.PERIODS, t['c0'])]
        _RESULTS[(name, wave)] = (ref.round_model(*m), t, R)
    return _RESULTS[(name, wave)]


# ---- 1. twin against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wave', sc.CASES)
def test_twin_against_the_longdouble_reference(twin, name, wave):
    _, t, R = _case(twin, name, wave)
    worst, own = dict.fromkeys(WHAT, 0.0), dict.fromkeys(WHAT, 0.0)
    for k, r in enumerate(R):
        assert np.isfinite(r['K'].astype(np.float64)).all() and np.isfinite(r['U']) and np.isfinite(r['dU_dT'])
        e, o = tol.errors(t, k, r)
        for w in WHAT:
            worst[w], own[w] = max(worst[w], e[w]), max(own[w], o[w])
    print('%s %s: ' % (name, wave) + ', '.join('%s %.2e (%.2e; reference %.2e)' % (w, v, tol.tolerance(w), own[w])
                                               for w, v in worst.items()))
    for w, v in worst.items():
        assert v <= tol.tolerance(w), (w, v, tol.tolerance(w))
        assert own[w] <= tol.REFERENCE_OWN[w] * 1.005, (w, own[w])                 # the recorded estimates hold
    if wave == 'love':
        assert np.all(t['K'][:, 1, :] == 0)                    # Love waves do not see vp: exactly 0
    assert np.all(t['K'][:, 0, -1] == 0)                       # the half-space has no thickness
    assert np.all(t['U'] < t['c']) and np.all(t['U'] > 0)      # normal dispersion in these models


def test_the_recorded_step_is_the_librarys_and_minimises_the_recorded_sweep():
    src = open(os.path.join(ROOT, 'bayhunter_amd', 'csrc', 'sens_group_core.h')).read()
    assert 'constexpr double SENS_GROUP_RG = 0x1p%d;' % tol.RG_LOG2 in src
    assert 'constexpr double SENS_GROUP_KAPPA = %.1f;' % tol.KAPPA_BOUND in src
    assert tol.KAPPA_MEASURED < max(tol.KAPPA_DRAWN.values()) <= tol.KAPPA_BOUND / 4      # the drawn models' range, with room
    assert sorted(tol.SWEEP) == list(range(6, 17))
    for col in (0, 2):                                         # K^U, dU/dT (U does not depend on the step)
        assert tol.SWEEP[-tol.RG_LOG2][col] == min(v[col] for v in tol.SWEEP.values())
    assert len({v[1] for v in tol.SWEEP.values()}) == 1
    for w in WHAT:                                             # twice the measured worst, above the reference's own
        assert tol.tolerance(w) == 2.0 * tol.MEASURED[w] >= tol.REFERENCE_OWN[w]
    assert max(tol.MEASURED[k] for k in KINDS) == tol.SWEEP[-tol.RG_LOG2][0]


def test_a_swept_step_moves_the_error_as_recorded(twin):
    """One line of the sweep again, on one case: K^U of L3, Rayleigh, with r_g at 2^-8, 2^-12 and 2^-16."""
    m, _, R = _case(twin, 'L3', 'rayleigh')
    errs = []
    for p in (8, 12, 16):
        t = twin.sensitivity(*m, sc.PERIODS, 'rayleigh', rg=2.0 ** -p)
        errs.append(max(max(tol.errors(t, k, r)[0][kind] for kind in KINDS) for k, r in enumerate(R)))
    # (the table holds three digits)
    assert errs[1] < errs[0] <= tol.SWEEP[8][0] * 1.005 and errs[1] < errs[2] <= tol.SWEEP[16][0] * 1.005


# ---- 2. identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wave', sc.CASES)
def test_scaling_identities(twin, name, wave):
    """U depends on (T, h, vp, vs, rho) through dimensionless groups only: scaling every density leaves U; scaling every
    velocity and every thickness by s at a fixed T scales U by s; scaling every thickness and T by s leaves U."""
    m = ref.round_model(*sc.MODELS[name])
    t = twin.sensitivity(*m, sc.PERIODS, wave)
    worst = tol.identities(m, t, sc.PERIODS)
    print('%s %s: ' % (name, wave) + ', '.join('%s %.2e (%.2e)' % (k, v, tol.identity_tolerance(k)) for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= tol.identity_tolerance(key), (key, v)


# ---- 3. the phase twin's bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,wave', sc.CASES)
def test_u_c_and_k_phase_are_the_phase_twins_bits(twin, name, wave):
    from bayhunter_amd import sensitivity as S
    m = sc.MODELS[name]
    t = twin.sensitivity(*m, sc.PERIODS, wave)
    p = twin.phase.sensitivity(*m, sc.PERIODS, wave)
    assert np.array_equal(t['c0'], p['c0']) and t['err'] == p['err'] == 0
    assert t['c'].tobytes() == p['c'].tobytes() and t['K_phase'].tobytes() == p['K'].tobytes()
    assert t['dc_dT'].tobytes() == p['dc_dT'].tobytes()
    assert t['U'].tobytes() == S.group_velocity(p['c'], p['dc_dT'], sc.PERIODS).tobytes()


# ---- 4. no value, zeros, refusals -------------------------------------------------------------------------------------------
def _all_nan(*xs):
    return all(np.isnan(x).all() for x in xs)


@pytest.mark.parametrize('wave', ['rayleigh', 'love'])
def test_rows_without_a_value_are_nan_together_and_padding_is_zero(twin, wave):
    m = ref.round_model(*sc.MODELS['L3'])
    t = twin.sensitivity(*m, sc.PERIODS, wave)
    h, vp, vs, rho = m
    pad = [np.concatenate([x, [np.nan, 1e30, -1.0]]) for x in m]           # never read
    K, U, dU, c, Kp = twin.row(*pad, sc.PERIODS, t['c0'], wave, nlay=3, Lmax=6)
    assert np.array_equal(K[:, :, :3], t['K']) and np.array_equal(U, t['U']) and np.array_equal(dU, t['dU_dT'])
    assert np.array_equal(c, t['c']) and np.array_equal(Kp[:, :, :3], t['K_phase'])
    assert np.all(K[:, :, 3:] == 0) and np.all(K[:, 0, 2] == 0) and np.all(Kp[:, :, 3:] == 0)
    assert np.isfinite(K).all() and np.any(K[:, 2, :3] != 0)
    assert 'water' in sc.NO_VALUE and _all_nan(*twin.row(h, vp, np.array([0., vs[1], vs[2]]), rho, sc.PERIODS, t['c0'], wave))
    assert 'flag' in sc.NO_VALUE and _all_nan(*twin.row(*m, sc.PERIODS, t['c0'], wave, err=1))
    assert _all_nan(*twin.row(*m, sc.PERIODS, t['c0'], wave, nlay=1))
    assert _all_nan(*twin.row(*pad, sc.PERIODS, t['c0'], wave, nlay=7, Lmax=6))
    assert {'c_zero', 'c_moved'} <= set(sc.NO_VALUE)
    for what, bad in (('c_zero', 0.0), ('c_moved', t['c0'][2] * (1 + 1e-5)), ('nan', np.nan), ('inf', np.inf), ('neg', -3.0)):
        cb = t['c0'].copy()
        cb[2] = bad
        K, U, dU, c, Kp = twin.row(*pad, sc.PERIODS, cb, wave, nlay=3, Lmax=6)
        assert _all_nan(K[2], U[2], dU[2], c[2], Kp[2]), what                         # all 4 Lmax entries, every output
        keep = [0, 1, 3, 4]
        assert np.array_equal(K[keep, :, :3], t['K'][keep]) and np.array_equal(U[keep], t['U'][keep]), what
    bad = twin.sensitivity([1., 0.], [np.nan, 6.], [np.nan, 3.5], [2.5, 2.8], sc.PERIODS, wave)
    assert bad['err'] != 0 and _all_nan(bad['K'], bad['U'], bad['dU_dT'], bad['c'], bad['K_phase'])


@pytest.mark.parametrize('wave', ['rayleigh', 'love'])
def test_a_rejected_side_root_leaves_the_whole_model_period_without_a_value(twin, wave):
    """The window of the side roots at a millionth of the library's (the tangent misses c(T+-) by kappa r_g^2 / 2, kappa
    some 0.1 here, against 64 in the window): the centre root stands, a side root is rejected, and U, c, dU/dT, K and
    K_phase are NaN together.  At the library's window, and at any wider one, every bit is the same."""
    m = ref.round_model(*sc.MODELS['L3'])
    t = twin.sensitivity(*m, sc.PERIODS, wave)
    lib_window = 0.5 * tol.KAPPA_BOUND * 2.0 ** (2 * tol.RG_LOG2)
    K, U, dU, c, Kp = twin.row(*m, sc.PERIODS, t['c0'], wave, window=1e-6 * lib_window)
    assert np.isfinite(twin.phase.row(*m, sc.PERIODS, t['c0'], wave)[1]).all()           # the phase pass has its c
    assert _all_nan(K, U, dU, c, Kp)
    for w in (lib_window, 1e-3):
        got = twin.row(*m, sc.PERIODS, t['c0'], wave, window=w)
        assert all(np.array_equal(a, b) for a, b in zip(got, (t['K'], t['U'], t['dU_dT'], t['c'], t['K_phase'])))
    # the tangent's miss is inside the window with the margin the derivation claims
    Kw, Uw, _, cw, _ = twin.row(*m, sc.PERIODS, t['c0'], wave, window=tol.KAPPA_MEASURED / tol.KAPPA_BOUND * lib_window)
    assert np.isfinite(cw).all() and np.array_equal(Kw, t['K'])


DRAW_PERIODS = np.linspace(1., 41., 21)


@pytest.mark.parametrize('wave', ['rayleigh', 'love'])
def test_drawn_models_lose_no_period_the_phase_pass_serves(twin, wave):
    """Ten-layer draws with vs increasing downward (the models of tools/sens_group_bench.py), 21 periods of 1 .. 41 s: the
    first 48 and the ten of the first 3072 whose curvature T^2 |c_TT| / c is 8 .. 10 (a slow top layer over fast rock,
    next to the Airy phase), which a window derived from the tuning list's curvature alone rejected
    (sens_group_tolerances.DRAWN_LOST).  Every (model, period) with a phase value has a group value, the curvature
    stays inside the recorded range, and the lost periods were genuine roots: a wider window returns the same bits."""
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(3072, 10, seed=1)
    worst = 0.0
    for b in list(range(48)) + sorted(tol.DRAWN_LOST):
        m = ref.round_model(*[x[b, :nl[b]] for x in (H, VP, VS, RHO)])
        t = twin.sensitivity(*m, DRAW_PERIODS, wave)
        p = twin.phase.sensitivity(*m, DRAW_PERIODS, wave)
        assert t['err'] == p['err'] == 0 and np.isfinite(p['c']).all() and np.isfinite(p['K']).all(), b
        for k in OUT_KEYS:
            assert np.isfinite(t[k]).all(), (b, k, np.nonzero(np.isnan(t['c']))[0])
        assert t['c'].tobytes() == p['c'].tobytes() and t['K_phase'].tobytes() == p['K'].tobytes()
        worst = max(worst, tol.kappa(t, DRAW_PERIODS))
        if b in tol.DRAWN_LOST:
            wide = twin.row(*m, DRAW_PERIODS, t['c0'], wave, window=2.0 ** -12)
            assert all(np.array_equal(a, t[k]) for a, k in zip(wide, OUT_KEYS)), b
            if wave == 'rayleigh':                              # the window this one replaced loses exactly that period
                old = twin.row(*m, DRAW_PERIODS, t['c0'], wave, window=4.0 * 2.0 ** (2 * tol.RG_LOG2))
                assert np.nonzero(np.isnan(old[3]))[0].tolist() == [tol.DRAWN_LOST[b]], b
    print('%s: kappa %.3g (recorded over 32 768 draws %.3g; bound %.0f)' % (wave, worst, tol.KAPPA_DRAWN[wave], tol.KAPPA_BOUND))
    assert worst <= tol.KAPPA_DRAWN[wave] * 1.005
    if wave == 'rayleigh':
        assert worst > 8.0                                      # the sample holds what the tuning list does not


def test_a_pool_without_a_group_target_is_refused_unless_a_ref_is_named():
    """pool_target on the targets alone (no device): the default of group_sensitivity() is the pool's only
    fundamental-mode group target; without one it is a ValueError, not a phase target served silently."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
    from bayhunter_amd import sensitivity as S
    from chain_scenario import joint_target
    data = os.path.join(ROOT, 'tests', 'golden', 'tutorial_observed')
    phase, group = joint_target(data, refs=('rdispph', 'prf')), joint_target(data, refs=('rdispgr', 'prf'))
    with pytest.raises(ValueError, match='no fundamental-mode group target'):
        S.pool_target(phase, None, 'group')
    wave, periods, tref = S.pool_target(phase, 'rdispph', 'group')                 # named: served
    assert (wave, tref) == ('rayleigh', 'rdispph') and np.array_equal(periods, phase.targets[0].obsdata.x)
    assert S.pool_target(group, None, 'group')[::2] == ('rayleigh', 'rdispgr')
    assert S.pool_target(phase, None)[::2] == ('rayleigh', 'rdispph')               # the phase default is as it was
    with pytest.raises(ValueError, match='group-velocity targets are not served'):
        S.pool_target(group, None)
    with pytest.raises(ValueError, match='no dispersion target'):
        S.pool_target(group, 'ldispgr', 'group')
    assert S.StationSensitivity.velocity == 'phase'


def test_c_abi_refuses_bad_arguments_before_it_touches_a_device(lib):
    from bayhunter_amd import _lib
    p = C.c_void_p(64)            # never dereferenced: every call below is refused first

    def batch(iwave=2, nper=5, flsph=0, c_stride=5, err_stride=1, null=None, Lmax=8, mstride=8, ws=1 << 20):
        a = [4, Lmax, mstride, p, p, p, p, p, iwave, nper, p, flsph, p, c_stride, p, err_stride, p, p, p, p, p, p, ws, None]
        if null is not None:
            a[null] = None
        return lib.bh_sens_group_batch(*a)
    assert batch(flsph=1) == _lib.BH_ERR_ARG and b'flsph' in lib.bh_last_error()
    for kw in (dict(iwave=0), dict(iwave=3), dict(nper=0), dict(nper=_lib.MAX_PERIODS + 1), dict(c_stride=4),
               dict(err_stride=0), dict(Lmax=0), dict(Lmax=_lib.MAX_LAYERS + 1), dict(mstride=7)) + tuple(
                   dict(null=i) for i in (3, 4, 5, 6, 7, 10, 12, 14, 16, 17, 18, 19)):
        assert batch(**kw) == _lib.BH_ERR_ARG, kw
        assert lib.bh_last_error()
    # K_phase may be NULL: the call then gets as far as the workspace check
    assert batch(ws=4 * 5 * 6 * 8 - 1) == _lib.BH_ERR_WORKSPACE and batch(null=21) == _lib.BH_ERR_WORKSPACE
    assert batch(null=20, ws=4 * 5 * 6 * 8 - 1) == _lib.BH_ERR_WORKSPACE
    assert lib.bh_sens_group_workspace_bytes(4, 5) == 6 * 160 and lib.bh_sens_group_workspace_bytes(65536, 21) == 6 * 65536 * 21 * 8
    assert lib.bh_sens_group_workspace_bytes(-1, 5) == 0
    f = np.ones(4, dtype=np.float32)
    t, K, x, err = np.linspace(1, 10, 61), np.zeros(61 * 16), np.zeros(61), C.c_int(0)

    def single(n=4, iflsph=0, iwave=2, kmax=5, null=None):
        a = [f.ctypes.data] * 4 + [n, iflsph, iwave, kmax, t.ctypes.data, K.ctypes.data, x.ctypes.data, x.ctypes.data,
                                   x.ctypes.data, K.ctypes.data, C.byref(err)]
        if null is not None:
            a[null] = None
        return lib.bh_group_sensitivity(*a)
    assert single(iflsph=1) == _lib.BH_ERR_ARG and b'flsph' in lib.bh_last_error()
    for kw in (dict(kmax=0), dict(kmax=61), dict(n=0), dict(n=101), dict(iwave=0), dict(iwave=3), dict(null=0), dict(null=3),
               dict(null=8), dict(null=9), dict(null=10), dict(null=11), dict(null=12), dict(null=14)):
        assert single(**kw) == _lib.BH_ERR_ARG, kw


def test_plugin_serves_every_dispersion_ref_and_refuses_what_the_pass_does_not():
    from bayhunter_amd import plugins
    m = sc.MODELS['L3']
    for r in ('rdispph', 'rdispgr', 'ldispph', 'ldispgr'):
        p = plugins.SurfDisp(sc.PERIODS, r)
        p.set_modelparams(mode=2)
        with pytest.raises(ValueError, match='mode'):
            p.group_sensitivity(*m)
        p.set_modelparams(mode=1, flsph=1)
        with pytest.raises(ValueError, match='flsph'):
            p.group_sensitivity(*m)
        with pytest.raises(ValueError, match='periods'):
            plugins.SurfDisp(np.linspace(1, 40, 61), r).group_sensitivity(*m)
    # the phase entry point still refuses a group ref
    with pytest.raises(ReferenceError, match='igr'):
        plugins.SurfDisp(sc.PERIODS, 'rdispgr').sensitivity(*m)


def test_python_entry_points_check_their_arguments_before_a_device():
    from bayhunter_amd import sensitivity as S
    with pytest.raises(ValueError, match='velocity'):
        S.summarize_sets(sc.PERIODS, 'rayleigh', np.zeros((4, 8)), [0, 4], 1.75, velocity='both')
    with pytest.raises(ValueError, match='wave'):
        S.group_batch(sc.PERIODS, *[np.zeros((1, 2))] * 4, [2], wave='stoneley')
    assert S.GROUP_REFS == {'rayleigh': 'rdispgr', 'love': 'ldispgr'}


# ---- 5. sanitizers ----------------------------------------------------------------------------------------------------------
def test_host_twin_under_asan_ubsan(tmp_path):
    """sens_group_core.h and the twin's own code as a stand-alone program (SENS_GROUP_SIM_MAIN) under AddressSanitizer and
    UBSan."""
    exe = str(tmp_path / 'sens_group_sim')
    c = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-omit-frame-pointer', '-DSENS_GROUP_SIM_MAIN', gc.SIM_SRCS[0], '-o', exe], capture_output=True, text=True)
    if c.returncode != 0 and ('cannot find' in c.stderr or 'sanitizer' in c.stderr.lower()):
        pytest.skip('sanitizer runtime not installed: ' + c.stderr[-300:])
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, UBSAN_OPTIONS='print_stacktrace=1'))
    if 'Shadow memory range interleaves' in r.stderr or 'ReserveShadowMemoryRange failed' in r.stderr:
        pytest.skip('the sanitizer runtime cannot start in this environment: ' + r.stderr[-300:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'sens group ok' in r.stdout and 'runtime error' not in r.stderr, r.stderr[-4000:]
