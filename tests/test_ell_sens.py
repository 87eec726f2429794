"""Ellipticity sensitivity kernels on the CPU: the host twin of ell_sens_root_kernel / ell_sens_kernel
(tests/hostsim/ell_sens_sim.cpp: ell_sens_core.h built with g++ and the device math) against

* the independent longdouble reference (tests/ell_sens_ref.py: no G_m + G_c dc/dm -- the root of every perturbed model
  solved again, the ellipticity evaluated there, then differenced) over sensitivity_cases.MODELS x PERIODS within
  tests/ell_sens_tolerances.py, and off that list within the bounds recorded there;
* itself with the other traction eliminated: the totals agree, the partial derivatives do not;
* the identities dimensional scaling gives any exact E(T, h, vp, vs, rho);
* the phase twin, bit for bit (c, K_phase), ell_core.h's value at the stored c, and itself with `absolute`;
* the rows without a value, the zeros, and the argument checks of the C ABI and of the Python entry points;
* itself under AddressSanitizer and UBSan, as a stand-alone program.
(What needs the device is in test_gpu_ell_sens.py.)
"""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

import ell_sens_cases as ec
import ell_sens_tolerances as tol
import sensitivity_cases as sc
import sensitivity_ref as ref
from conftest import ROOT

KINDS = tol.KINDS
OUT_KEYS = ('K', 'E', 'dE_dT', 'c', 'K_phase')
NAMES = list(sc.MODELS)


@pytest.fixture(scope='module')
def twin():
    return ec.load_sim()


_REF = {}


def _references(twin):
    """The twin and the reference of every case on and off the list, computed once (the reference in a few processes)
    and not changed: name -> (twin dict, list of the reference's dicts per period)."""
    if not _REF:
        tasks, keys = [], []
        for name in NAMES + list(sc.OFFLIST):
            on = name in sc.MODELS
            m, periods = (sc.MODELS[name], sc.PERIODS) if on else (sc.OFFLIST[name], sc.OFFLIST_PERIODS)
            t = twin.sensitivity(*m, periods)
            assert t['err'] == 0 and np.all(t['c0'] > 0)
            _REF[name] = (t, [])
            for k, (T, c0) in enumerate(zip(periods, t['c0'])):
                tasks.append((m, T, c0, None if on else tol.subset(t['K'][k], len(m[0]))))
                keys.append(name)
        with mp.get_context('fork').Pool(min(8, os.cpu_count() or 1)) as pool:
            for name, r in zip(keys, pool.map(tol._ref_task, tasks, chunksize=1)):
                _REF[name][1].append(r)
    return _REF


def _worst(t, R, periods):
    worst, own = dict.fromkeys(tol.WHAT, 0.0), dict.fromkeys(tol.WHAT, 0.0)
    for k, r in enumerate(R):
        assert np.isfinite(r['K'].astype(np.float64)[~np.isnan(r['K'].astype(np.float64))]).all()
        assert np.isfinite(r['E']) and np.isfinite(r['dE_dT'])
        e, o = tol.errors(t, k, r, periods[k])
        for w in tol.WHAT:
            worst[w], own[w] = max(worst[w], e[w]), max(own[w], o[w])
    return worst, own


# ---- 3. twin against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_twin_against_the_longdouble_reference(twin, name):
    t, R = _references(twin)[name]
    worst, own = _worst(t, R, sc.PERIODS)
    print('%s: ' % name + ', '.join('%s %.2e (%.2e; reference %.2e)' % (w, v, tol.tolerance(w), own[w]) for w, v in worst.items()))
    for w, v in worst.items():
        assert v <= tol.tolerance(w), (w, v, tol.tolerance(w))
        assert own[w] <= tol.REFERENCE_OWN[w] * 1.005, (w, own[w])                 # the recorded estimates hold
    assert np.all(t['K'][:, 0, -1] == 0)                       # the half-space has no thickness
    assert np.isfinite(t['K']).all() and np.all(np.abs(t['K'][:, 2, :]).max(axis=1) > 0)


def test_the_recorded_steps_are_the_librarys_and_the_tolerances_follow_the_measurements():
    src = open(os.path.join(ROOT, 'bayhunter_amd', 'csrc', 'ell_sens_core.h')).read()
    phase = open(os.path.join(ROOT, 'bayhunter_amd', 'csrc', 'sens_core.h')).read()
    line = 's.c = 0x1p%d; s.t = 0x1p%d; s.h = 0x1p%d; s.v = 0x1p%d; s.rho = 0x1p%d;' % tuple(tol.STEPS_LOG2[s] for s in tol.STEP_ORDER)
    assert line in src and line in phase
    for s in tol.STEP_ORDER:                                    # five lines of the sweep per step, the library's among them
        assert sorted(p for (k, p) in tol.SWEEP if k == s) == [tol.STEPS_LOG2[s] + d for d in (-4, -2, 0, 2, 4)]
        assert tol.SWEEP[(s, tol.STEPS_LOG2[s])] == (max(tol.MEASURED[k] for k in KINDS), tol.MEASURED['dE_dT'])
    for w in tol.WHAT:
        assert tol.tolerance(w) == max(4.0 * tol.MEASURED[w], tol.REFERENCE_OWN[w]) >= tol.REFERENCE_OWN[w]
        assert tol.offlist_bound(w) == 4.0 * tol.OFFLIST_MEASURED[w]


@pytest.mark.parametrize('name', list(sc.OFFLIST))
def test_twin_against_the_reference_off_the_list(twin, name):
    """Nothing was tuned on these models: the worst error is finite and below the bound recorded next to its measured
    value (ell_sens_tolerances.OFFLIST_MEASURED)."""
    t, R = _references(twin)[name]
    worst, _ = _worst(t, R, sc.OFFLIST_PERIODS)
    print('%s: ' % name + ', '.join('%s %.2e (%.2e)' % (w, v, tol.offlist_bound(w)) for w, v in worst.items()))
    assert all(np.isfinite(t[k]).all() for k in OUT_KEYS)
    for w, v in worst.items():
        assert np.isfinite(v) and v <= tol.offlist_bound(w), (w, v)


def test_a_swept_step_moves_the_error_as_recorded(twin):
    """Two lines of the sweep again: the density step at 2^-24 and the step over T at 2^-12, over the whole list."""
    refs = _references(twin)
    for s, p, col in (('rho', -24, 0), ('t', -12, 1)):
        steps = [2.0 ** (p if k == s else tol.STEPS_LOG2[k]) for k in tol.STEP_ORDER]
        worst = 0.0
        for name in NAMES:
            t = twin.sensitivity(*sc.MODELS[name], sc.PERIODS, steps=steps)
            w, _ = _worst(t, refs[name][1], sc.PERIODS)
            worst = max(worst, max(w[k] for k in KINDS) if col == 0 else w['dE_dT'])
        base = tol.SWEEP[(s, tol.STEPS_LOG2[s])][col]
        assert 2 * base < worst <= tol.SWEEP[(s, p)][col] * 1.005, (s, p, worst)           # (the table holds three digits)


# ---- 4. both eliminations ---------------------------------------------------------------------------------------------------
def test_both_eliminations_give_the_same_total_and_different_partial_derivatives(twin):
    """ELL_FORM_TR and ELL_FORM_TZ differ off the root and agree along it: the totals G_m + G_c dc/dm agree within the
    tolerance of the reference comparison; with the G_c dc/dm term left out they disagree by more than 100 tolerances
    on at least one case (here: on every model) -- the comparison can fail."""
    far = 0
    for name in NAMES:
        m = sc.MODELS[name]
        tz, tr = twin.sensitivity(*m, sc.PERIODS), twin.sensitivity(*m, sc.PERIODS, form='tr')
        d = tol.form_differences(tz, tr, sc.PERIODS)
        print(name, {w: float('%.2e' % v) for w, v in d.items()})
        for w, v in d.items():
            assert v <= tol.tolerance(w), (name, w, v)
            assert v <= tol.FORMS_MEASURED[w] * 1.005, (name, w, v)
        assert tz['c'].tobytes() == tr['c'].tobytes() and tz['K_phase'].tobytes() == tr['K_phase'].tobytes()
        pz, pr = twin.sensitivity(*m, sc.PERIODS, total=False), twin.sensitivity(*m, sc.PERIODS, form='tr', total=False)
        p = tol.form_differences(pz, pr, sc.PERIODS)
        far += any(p[k] > 100 * tol.tolerance(k) for k in KINDS)
        assert all(p[k] <= tol.PARTIAL_FORMS[k] * 1.005 for k in KINDS)
    assert far >= 1
    assert far == len(NAMES)


# ---- 5. identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_scaling_identities(twin, name):
    """E is a ratio and depends on (T, h, vp, vs, rho) through dimensionless groups only: scaling every density leaves
    E; scaling every velocity by s leaves E at the period T / s; scaling every thickness by s leaves E at s T."""
    m = ref.round_model(*sc.MODELS[name])
    t = twin.sensitivity(*m, sc.PERIODS)
    worst = tol.identities(m, t, sc.PERIODS)
    print('%s: ' % name + ', '.join('%s %.2e (%.2e)' % (k, v, tol.identity_tolerance(k)) for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= tol.identity_tolerance(key), (key, v)


# ---- 6. the existing passes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES + ['sediment'])
def test_c_and_k_phase_are_the_phase_twins_bits_and_e_is_the_value_at_the_stored_c(twin, name):
    m, periods = (ec.SEDIMENT, ec.SEDIMENT_PERIODS) if name == 'sediment' else (sc.MODELS[name], sc.PERIODS)
    t = twin.sensitivity(*m, periods)
    p = twin.phase.sensitivity(*m, periods, 'rayleigh')
    assert np.array_equal(t['c0'], p['c0']) and t['err'] == p['err'] == 0
    assert t['c'].tobytes() == p['c'].tobytes() and t['K_phase'].tobytes() == p['K'].tobytes()
    # E is G at the polished root; ell_kernel's value is G at the stored real*4 c
    v = twin.value(*m, periods, t['c0'])
    first = np.abs(t['G_c']) * np.abs(t['c'] - t['c0'])
    excess = (np.abs(t['E'] - v) - first) / np.abs(t['E'])
    print(name, 'E - value', np.abs(t['E'] - v).max(), 'first order', first.max(), 'excess', excess.max())
    assert np.all(excess <= tol.STORED_C_BOUND)
    if name != 'sediment':
        assert excess.max() <= max(tol.STORED_C_MEASURED * 1.005, 0.0)
    assert np.abs(t['c'] - t['c0']).max() > 0                  # the polish moved the root: the two values are not one


def test_absolute_flips_exactly_the_periods_of_prograde_motion(twin):
    """The list has no E < 0 (checked here), so ell_sens_cases.SEDIMENT supplies the prograde window."""
    for name in NAMES:
        s, a = twin.sensitivity(*sc.MODELS[name], sc.PERIODS), twin.sensitivity(*sc.MODELS[name], sc.PERIODS, absolute=True)
        assert np.all(s['E'] > 0) and all(s[k].tobytes() == a[k].tobytes() for k in OUT_KEYS), name
    s = twin.sensitivity(*ec.SEDIMENT, ec.SEDIMENT_PERIODS)
    a = twin.sensitivity(*ec.SEDIMENT, ec.SEDIMENT_PERIODS, absolute=True)
    neg = s['E'] < 0
    assert neg.any() and (~neg).any() and s['err'] == 0 and np.isfinite(s['K']).all()
    assert np.all(a['E'] > 0)
    for k in ('K', 'E', 'dE_dT'):
        assert np.array_equal(a[k][neg], -s[k][neg]) and np.array_equal(a[k][~neg], s[k][~neg]), k
    for k in ('c', 'K_phase'):
        assert a[k].tobytes() == s[k].tobytes()
    # the reference agrees about the sign and the size at the prograde period
    k = int(np.nonzero(neg)[0][0])
    import ell_sens_ref
    r = ell_sens_ref.kernels(*ec.SEDIMENT, ec.SEDIMENT_PERIODS[k], s['c0'][k], slots=[(2, 0), (0, 0)])
    assert r['E'] < 0 and abs(s['E'][k] - r['E']) <= 1e-12 * abs(r['E'])
    for ki, i in ((2, 0), (0, 0)):
        assert abs(s['K'][k, ki, i] - r['K'][ki, i]) <= tol.offlist_bound(KINDS[ki]) * np.abs(s['K'][k, ki]).max()


# ---- 7. no value ------------------------------------------------------------------------------------------------------------
def _all_nan(*xs):
    return all(np.isnan(x).all() for x in xs)


def test_rows_without_a_value_are_nan_together_and_padding_is_zero(twin):
    m = ref.round_model(*sc.MODELS['L3'])
    t = twin.sensitivity(*m, sc.PERIODS)
    h, vp, vs, rho = m
    pad = [np.concatenate([x, [np.nan, 1e30, -1.0]]) for x in m]           # never read
    K, E, dE, c, Kp = twin.row(*pad, sc.PERIODS, t['c0'], nlay=3, Lmax=6)
    assert np.array_equal(K[:, :, :3], t['K']) and np.array_equal(E, t['E']) and np.array_equal(dE, t['dE_dT'])
    assert np.array_equal(c, t['c']) and np.array_equal(Kp[:, :, :3], t['K_phase'])
    assert np.all(K[:, :, 3:] == 0) and np.all(K[:, 0, 2] == 0) and np.all(Kp[:, :, 3:] == 0)
    assert np.isfinite(K).all() and np.any(K[:, 2, :3] != 0)
    without = twin.row(*pad, sc.PERIODS, t['c0'], nlay=3, Lmax=6, k_phase=False)
    assert all(np.array_equal(a, b) for a, b in zip(without[:4], (K, E, dE, c))) and np.all(without[4] == 0)
    assert sc.NO_VALUE == ('water', 'flag', 'c_zero', 'c_moved')
    assert _all_nan(*twin.row(h, vp, np.array([0., vs[1], vs[2]]), rho, sc.PERIODS, t['c0']))           # water
    assert _all_nan(*twin.row(*m, sc.PERIODS, t['c0'], err=1))                                         # flag
    assert _all_nan(*twin.row(*m, sc.PERIODS, t['c0'], nlay=1))                                        # a half-space alone
    assert _all_nan(*twin.row(*pad, sc.PERIODS, t['c0'], nlay=7, Lmax=6))
    for what, bad in (('c_zero', 0.0), ('c_moved', t['c0'][2] * (1 + 1e-5)), ('nan', np.nan), ('inf', np.inf), ('neg', -3.0)):
        cb = t['c0'].copy()
        cb[2] = bad
        K, E, dE, c, Kp = twin.row(*pad, sc.PERIODS, cb, nlay=3, Lmax=6)
        assert _all_nan(K[2], E[2], dE[2], c[2], Kp[2]), what                         # all 4 Lmax entries, every output
        keep = [0, 1, 3, 4]
        assert np.array_equal(K[keep, :, :3], t['K'][keep]) and np.array_equal(E[keep], t['E'][keep]), what
    bad = twin.sensitivity([1., 0.], [np.nan, 6.], [np.nan, 3.5], [2.5, 2.8], sc.PERIODS)
    assert bad['err'] != 0 and _all_nan(*[bad[k] for k in OUT_KEYS])


# ---- 8. without a device ----------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_before_it_touches_a_device(lib):
    from bayhunter_amd import _lib
    p = C.c_void_p(64)            # never dereferenced: every call below is refused first

    def batch(B=4, nper=5, flsph=0, c_stride=5, err_stride=1, null=None, Lmax=8, mstride=8, ws=1 << 20):
        a = [B, Lmax, mstride, p, p, p, p, p, nper, p, flsph, 1, p, c_stride, p, err_stride, p, p, p, p, p, p, ws, None]
        if null is not None:
            a[null] = None
        return lib.bh_ell_sens_batch(*a)
    assert batch(flsph=1) == _lib.BH_ERR_ARG and b'flsph' in lib.bh_last_error()
    assert batch(nper=_lib.MAX_PERIODS + 1) == _lib.BH_ERR_ARG and b'nper' in lib.bh_last_error()
    for kw in (dict(nper=0), dict(nper=_lib.MAX_PERIODS + 1), dict(c_stride=4), dict(err_stride=0), dict(Lmax=0),
               dict(Lmax=_lib.MAX_LAYERS + 1), dict(mstride=7), dict(B=-1)) + tuple(
                   dict(null=i) for i in (3, 4, 5, 6, 7, 9, 12, 14, 16, 17, 18, 19)):
        assert batch(**kw) == _lib.BH_ERR_ARG, kw
        assert lib.bh_last_error()
    # a launch that does not fit: 2^31 - 1 models of 100 layers at 60 periods are more than 2^31 - 1 workgroups
    assert batch(B=0x7fffffff, Lmax=100, mstride=100, nper=60, c_stride=60, ws=1 << 62) == _lib.BH_ERR_ARG
    assert b'do not fit' in lib.bh_last_error()
    # K_phase may be NULL: the call then gets as far as the workspace check
    assert batch(ws=4 * 5 * 3 * 8 - 1) == _lib.BH_ERR_WORKSPACE and batch(null=21) == _lib.BH_ERR_WORKSPACE
    assert batch(null=20, ws=4 * 5 * 3 * 8 - 1) == _lib.BH_ERR_WORKSPACE
    assert batch(B=0) == _lib.BH_OK
    assert lib.bh_ell_sens_workspace_bytes(4, 5) == 3 * 160 and lib.bh_ell_sens_workspace_bytes(65536, 21) == 3 * 65536 * 21 * 8
    assert lib.bh_ell_sens_workspace_bytes(-1, 5) == 0
    # the layer total of the ensemble reduction
    def total(B=4, Lmax=8, nper=5, q_stride=8, null=None):
        a = [B, Lmax, nper, p, p, q_stride, 0.32, p, None]
        if null is not None:
            a[null] = None
        return lib.bh_ell_sens_vs_total(*a)
    for kw in (dict(B=-1), dict(Lmax=0), dict(Lmax=_lib.MAX_LAYERS + 1), dict(nper=0), dict(nper=_lib.MAX_PERIODS + 1),
               dict(q_stride=7), dict(null=3), dict(null=4), dict(null=7)):
        assert total(**kw) == _lib.BH_ERR_ARG, kw
        assert lib.bh_last_error()
    assert total(B=0x7fffffff, Lmax=100, q_stride=100, nper=60) == _lib.BH_ERR_ARG and b'do not fit' in lib.bh_last_error()
    assert total(B=0) == _lib.BH_OK
    f = np.ones(4, dtype=np.float32)
    t, K, x, err = np.linspace(1, 10, 61), np.zeros(61 * 16), np.zeros(61), C.c_int(0)

    def single(n=4, iflsph=0, kmax=5, null=None):
        a = [f.ctypes.data] * 4 + [n, iflsph, 1, kmax, t.ctypes.data, K.ctypes.data, x.ctypes.data, x.ctypes.data,
                                   x.ctypes.data, K.ctypes.data, C.byref(err)]
        if null is not None:
            a[null] = None
        return lib.bh_ellipticity_sensitivity(*a)
    assert single(iflsph=1) == _lib.BH_ERR_ARG and b'flsph' in lib.bh_last_error()
    for kw in (dict(kmax=0), dict(kmax=61), dict(n=0), dict(n=101), dict(null=0), dict(null=3), dict(null=8), dict(null=9),
               dict(null=10), dict(null=11), dict(null=12), dict(null=14)):
        assert single(**kw) == _lib.BH_ERR_ARG, kw


def _joint(flsph=0, absolute=True, with_ell=True, extra=()):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
    from bayhunter_amd import targets as T
    data = os.path.join(ROOT, 'tests', 'golden', 'tutorial_observed')
    d = np.loadtxt(os.path.join(data, 'st3_rdispph.dat'))
    out = [T.RayleighDispersionPhase(d[:, 0], d[:, 1])]
    if with_ell:
        out.append(T.RayleighEllipticity(d[:, 0], np.full(d.shape[0], 0.8)))
        out[-1].moddata.plugin.set_modelparams(flsph=flsph, absolute=absolute)
    for r in extra:
        out.append(T.RayleighEllipticity(d[::2, 0], np.full(d[::2].shape[0], 0.8)))
    p = np.loadtxt(os.path.join(data, 'st3_prf.dat'))
    out.append(T.PReceiverFunction(p[:, 0], p[:, 1]))
    return T.JointTarget(out), d[:, 0]


def test_pool_target_picks_the_ellipticity_target():
    """pool_target on the targets alone (no device)."""
    from bayhunter_amd import sensitivity as S, targets as T
    joint, x = _joint()
    wave, periods, tref = S.pool_target(joint, None, 'ellipticity')
    assert (wave, tref) == ('rayleigh', 'rellip') and np.array_equal(periods, x)
    assert S.pool_target(joint, 'rellip', 'ellipticity')[2] == 'rellip'
    assert S._pool_absolute(joint, 'rellip', 'ellipticity') is True
    assert S._pool_absolute(_joint(absolute=False)[0], 'rellip', 'ellipticity') is False
    assert S.pool_target(joint, None)[::2] == ('rayleigh', 'rdispph')               # the phase default is as it was
    with pytest.raises(ValueError, match='no ellipticity target'):
        S.pool_target(_joint(with_ell=False)[0], None, 'ellipticity')
    with pytest.raises(ValueError, match='no ellipticity target'):
        S.pool_target(joint, 'rdispph', 'ellipticity')
    with pytest.raises(ValueError, match='flsph'):
        S.pool_target(_joint(flsph=1)[0], None, 'ellipticity')
    with pytest.raises(ValueError, match='ref is one of'):
        S.pool_target(_joint(extra=('second',))[0], None, 'ellipticity')
    with pytest.raises(ValueError, match='periods'):                               # more than 60: no such target exists
        S.pool_target(T.JointTarget([T.RayleighEllipticity(np.linspace(1, 40, 61), np.full(61, 0.8))]), None, 'ellipticity')
    assert S.VELOCITIES == ('phase', 'group', 'ellipticity')


def test_python_entry_points_check_their_arguments_before_a_device():
    from bayhunter_amd import plugins, sensitivity as S
    models = np.zeros((4, 8))
    with pytest.raises(ValueError, match='velocity'):
        S.summarize_sets(sc.PERIODS, 'rayleigh', models, [0, 4], 1.75, velocity='hv')
    with pytest.raises(ValueError, match="the ellipticity is the Rayleigh wave's"):
        S.summarize_sets(sc.PERIODS, 'love', models, [0, 4], 1.75, velocity='ellipticity')
    with pytest.raises(ValueError, match='wave'):
        S.summarize(sc.PERIODS, 'stoneley', models, 1.75, velocity='ellipticity')
    with pytest.raises(ValueError, match="target 'rellip' has more than 60 periods"):
        S.summarize_sets(np.linspace(1, 40, 61), 'rayleigh', models, [0, 4], 1.75, velocity='ellipticity')
    with pytest.raises(ValueError, match='kind'):
        S.summarize_sets(sc.PERIODS, 'rayleigh', models, [0, 4], 1.75, kind='h', velocity='ellipticity')
    with pytest.raises(ValueError, match='one per row'):
        S.summarize_sets(sc.PERIODS, 'rayleigh', models, [0, 4], [1.75] * 3, velocity='ellipticity')
    with pytest.raises(ValueError, match='max_rows'):
        S.summarize_sets(sc.PERIODS, 'rayleigh', models, [0, 4], 1.75, max_rows=0, velocity='ellipticity')
    p = plugins.RayleighEllipticity(sc.PERIODS)
    p.set_modelparams(flsph=1)
    with pytest.raises(ValueError, match='flsph'):
        p.sensitivity(*sc.MODELS['L3'])


# ---- sanitizers -------------------------------------------------------------------------------------------------------------
def test_host_twin_under_asan_ubsan(tmp_path):
    """ell_sens_core.h and the twin's own code as a stand-alone program (ELL_SENS_SIM_MAIN) under AddressSanitizer and
    UBSan."""
    exe = str(tmp_path / 'ell_sens_sim')
    c = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-omit-frame-pointer', '-DELL_SENS_SIM_MAIN', ec.SIM_SRCS[0], '-o', exe], capture_output=True, text=True)
    if c.returncode != 0 and ('cannot find' in c.stderr or 'sanitizer' in c.stderr.lower()):
        pytest.skip('sanitizer runtime not installed: ' + c.stderr[-300:])
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, UBSAN_OPTIONS='print_stacktrace=1'))
    if 'Shadow memory range interleaves' in r.stderr or 'ReserveShadowMemoryRange failed' in r.stderr:
        pytest.skip('the sanitizer runtime cannot start in this environment: ' + r.stderr[-300:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'ell sens ok' in r.stdout and 'runtime error' not in r.stderr, r.stderr[-4000:]
