"""Rayleigh-wave ellipticity (H/V) on the CPU: the host twin of ell_kernel (tests/hostsim/ell_sim.cpp: ell_core.h
built with g++ and the device math) against

* the closed form of the homogeneous half-space, derived from the Rayleigh equation (ellipticity_ref.rayleigh_root,
  half_space_hv), for Vp/Vs = sqrt 3, 1.6 and 2.2 and 1, 21 and 60 periods;
* the independent longdouble reference (tests/ellipticity_ref.py: Thomson-Haskell 4-vectors, no compound matrices) at
  the phase velocity the twin's search returned, over ellipticity_cases.CASES with flsph 0 and 1, within
  tests/ellipticity_tolerances.py;
* itself: the two quotients of Dunkin's vector agree within what the search's stopping tolerance allows, and each is the
  elimination of the reference it is named after; the layer-by-layer earth flattening returns swd_sphere's bits;
* the conditions for a NaN, the row layout with ellipticity targets, and the argument checks of the C ABI.
"""
import ctypes as C

import numpy as np
import pytest

import ellipticity_cases as ec
import ellipticity_ref as ref
import ellipticity_tolerances as tol


@pytest.fixture(scope='module')
def twin():
    return ec.load_sim()


_RESULTS = {}


def _case(twin, name, fl):
    """Twin and reference of one case, computed once: (periods, c, twin tz, twin tr, ref tz, ref tr)."""
    if (name, fl) not in _RESULTS:
        (h, vp, vs, rho), per = ec.CASES[name]
        ell, c, err = twin.ellipticity(h, vp, vs, rho, per, fl)
        assert err == 0 and np.all(c > 0)
        m32 = [np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64) for x in (h, vp, vs, rho)]
        tz = twin.row(*m32, per, c, flsph=fl, form=ec.FORM_TZ)
        tr = twin.row(*m32, per, c, flsph=fl, form=ec.FORM_TR)
        assert np.array_equal(tz, ell)                      # es_ellipticity is the search followed by the row
        _RESULTS[(name, fl)] = (per, c, tz, tr, ref.ellipticity(h, vp, vs, rho, per, c, 'tz', fl),
                                ref.ellipticity(h, vp, vs, rho, per, c, 'tr', fl))
    return _RESULTS[(name, fl)]


def _scale(r):
    return np.maximum(np.abs(np.asarray(r, dtype=np.float64)), tol.ELL_FLOOR)


def _relerr(got, want):
    return np.abs((got - want).astype(np.float64)) / _scale(want)


# ---- the homogeneous half-space -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('vpvs', [np.sqrt(3.), 1.6, 2.2])
@pytest.mark.parametrize('periods', [np.array([10.]), ec.PER21, np.linspace(1., 60., 60)], ids=['1', '21', '60'])
def test_layer_over_identical_half_space_gives_the_closed_form(twin, vpvs, periods):
    vs = np.float32(3.5)
    vp = np.float32(3.5 * vpvs)
    ell, c, err = twin.ellipticity([10., 0.], [vp, vp], [vs, vs], [2.8, 2.8], periods)
    assert err == 0
    cr = ref.rayleigh_root(vp, vs)
    want = ref.half_space_hv(vp, vs, cr)
    if vpvs == np.sqrt(3.):
        assert abs(float(cr) / float(vs) - 0.9194) < 1e-4 and abs(float(want) - 0.6812) < 1e-4      # the textbook values
    delta = tol.SEARCH_RTOL * cr
    assert np.all(np.abs(c - float(cr)) <= float(delta))     # the search's c is where its stopping rule puts it
    # at the same c the closed form with the normal traction eliminated is the same function: rounding only
    same_c = np.array([ref.half_space_hv(vp, vs, ci) for ci in c])
    e_same = _relerr(ell, same_c).max()
    # against the half-space's own value the distance is the slope of that function times |c - cr| <= delta
    slope = abs(ref.half_space_hv(vp, vs, cr + delta) - ref.half_space_hv(vp, vs, cr - delta))
    e_root = np.abs((ell - want).astype(np.float64)).max()
    print('vp/vs %.3f: |twin - closed form at c| %.3e (bound %.3e), |twin - closed form at the root| %.3e (bound %.3e)'
          % (vpvs, e_same, tol.ELL_RTOL, e_root, float(slope) + tol.ELL_RTOL * float(want)))
    assert e_same <= tol.ELL_RTOL
    assert e_root <= float(slope) + tol.ELL_RTOL * float(want)
    assert np.all(ell > 0)                                    # retrograde


def test_the_reference_gives_the_closed_form_on_a_half_space():
    vp, vs = np.float32(3.5 * np.sqrt(3.)), np.float32(3.5)
    cr = ref.rayleigh_root(vp, vs)
    for elim in ('tz', 'tr'):
        got = ref.ellipticity([10., 5., 0.], [vp] * 3, [vs] * 3, [2.8] * 3, [3., 20.], [cr, cr], elim)
        assert np.abs(got - ref.half_space_hv(vp, vs, cr)).max() < 1e-16


# ---- the case list ------------------------------------------------------------------------------------------------------
CASE_IDS = [(n, fl) for n in ec.CASES for fl in (0, 1)]


def _excluded(name, fl, per, c, rel=1.0e-6, eliminate='tz'):
    h, vp, vs, rho = ec.CASES[name][0]
    return np.array([ref.vertical_changes_sign(h, vp, vs, rho, t, ci, rel, fl, eliminate) for t, ci in zip(per, c)])


def test_the_case_list_covers_what_it_should_and_stays_inside_the_exclusion_cap(twin):
    assert sorted(len(ec.CASES[n][0][0]) for n in ('L2', 'L3', 'L5', 'L10', 'L31')) == [2, 3, 5, 10, 31]
    vs = ec.CASES['lvz'][0][2]
    assert np.any(np.diff(vs) < 0)                            # a low-velocity zone
    per, c, tz, _, rz, _ = _case(twin, 'sediment', 0)
    assert np.any(rz < 0) and np.any(rz > 0)                  # a prograde window inside the band
    total = excluded = 0
    for name, fl in CASE_IDS:
        per, c = _case(twin, name, fl)[:2]
        excluded += int(_excluded(name, fl, per, c).sum())
        total += per.size
    print('%d of %d (model, period) pairs lie within 1e-6 c of a zero of Uz' % (excluded, total))
    assert excluded <= tol.EXCLUDED_CAP * total


@pytest.mark.parametrize('name,fl', CASE_IDS)
def test_twin_against_the_longdouble_reference(twin, name, fl):
    per, c, tz, tr, rz, rr = _case(twin, name, fl)
    keep = ~_excluded(name, fl, per, c)
    e_tz, e_tr = _relerr(tz, rz)[keep].max(), _relerr(tr, rz)[keep].max()
    print('%s flsph %d: ELL_FORM_TZ %.3e, ELL_FORM_TR %.3e against the reference (zero normal traction); bound %.3e'
          % (name, fl, e_tz, e_tr, tol.ELL_RTOL))
    assert e_tz <= tol.ELL_RTOL
    assert e_tz < e_tr                                        # the form the library takes is the better one
    assert np.array_equal(np.signbit(tz[keep]), np.signbit(np.asarray(rz, dtype=np.float64)[keep]))


@pytest.mark.parametrize('name,fl', CASE_IDS)
def test_the_two_forms_agree_within_the_searchs_tolerance(twin, name, fl):
    """D(c) = tz(c) - tr(c) vanishes at the exact root c*, |c - c*| <= delta = SEARCH_RTOL c, and is monotone over an
    interval that short unless a pole lies in it: |D(c)| <= |D(c + delta) - D(c - delta)|, evaluated on the reference.
    Each form carries its own rounding error on top.  The other form is the reference's other elimination."""
    per, c, tz, tr, rz, rr = _case(twin, name, fl)
    (h, vp, vs, rho) = ec.CASES[name][0]
    keep = ~(_excluded(name, fl, per, c, 4e-6, 'tz') | _excluded(name, fl, per, c, 4e-6, 'tr'))
    assert keep.sum() >= 0.9 * per.size
    # which elimination the other form is: at every period orders of magnitude closer to 'tr' than to 'tz' (its own
    # rounding error was not measured: next to its pole it is 2e-12, elsewhere 1e-15, against 1e-5 .. 1e-2)
    assert np.all(_relerr(tr, rr)[keep] <= np.maximum(1e-3 * _relerr(tr, rz)[keep], tol.ELL_RTOL))
    d = c * tol.SEARCH_RTOL
    D = [ref.ellipticity(h, vp, vs, rho, per, cc, 'tz', fl) - ref.ellipticity(h, vp, vs, rho, per, cc, 'tr', fl)
         for cc in (c + d, c - d)]
    bound = np.abs((D[0] - D[1]).astype(np.float64)) + 2 * tol.ELL_RTOL * _scale(rz)
    diff = np.abs(tz - tr)
    print('%s flsph %d: max |tz - tr| %.3e, smallest bound / difference %.2f' % (name, fl, diff[keep].max(),
                                                                               (bound[keep] / diff[keep]).min()))
    assert np.all(diff[keep] <= bound[keep])


def test_absolute_flag_and_prograde_window(twin):
    (h, vp, vs, rho), per = ec.CASES['sediment']
    signed, c, _ = twin.ellipticity(h, vp, vs, rho, per, 0, absolute=False)
    absolute, c2, _ = twin.ellipticity(h, vp, vs, rho, per, 0, absolute=True)
    assert np.array_equal(c, c2) and np.array_equal(absolute, np.abs(signed))
    neg = np.nonzero(signed < 0)[0]
    assert neg.size > 3 and np.all(np.diff(neg) == 1) and neg[0] > 0 and neg[-1] < per.size - 1      # one window


@pytest.mark.parametrize('name', list(ec.CASES))
def test_layer_by_layer_flattening_is_swd_sphere(twin, name):
    (h, vp, vs, rho), per = ec.CASES[name]
    c = _case(twin, name, 1)[1]
    a = twin.row(h, vp, vs, rho, per, c, flsph=1, sphere_path=0)
    b = twin.row(h, vp, vs, rho, per, c, flsph=1, sphere_path=1)
    assert np.array_equal(a, b) and not np.array_equal(a, twin.row(h, vp, vs, rho, per, c, flsph=0))


def test_reference_flattening_is_the_twins():
    """ellipticity_ref.flatten_rayleigh restates surfdisp96.f's `sphere`; the twin's is the library's swd_sphere, whose
    results the dispersion tests hold to the reference program.  At flsph = 1 the reference above matched the twin to
    1e-14, which no model rounded differently to real*4 (6e-8) would."""
    h, vp, vs, rho = ec.CASES['L31'][0]
    d, a, b, r = ref.flatten_rayleigh(h, vp, vs, rho)
    assert d[-1] == 0 and np.all(d[:-1] > np.asarray(h, dtype=np.float32)[:-1]) and np.all(a > vp) and np.all(r < rho)


# ---- NaN ----------------------------------------------------------------------------------------------------------------
def test_rows_without_an_ellipticity_are_nan(twin):
    (h, vp, vs, rho), per = ec.CASES['L5']
    c = _case(twin, 'L5', 0)[1]
    good = twin.row(h, vp, vs, rho, per, c)
    assert np.all(np.isfinite(good))
    water_vs = np.array(vs)
    water_vs[0] = 0.0
    assert np.all(np.isnan(twin.row(h, vp, water_vs, rho, per, c)))                    # llw != 1
    assert np.all(np.isnan(twin.row(h, vp, vs, rho, per, c, nlay=1)))                  # a half-space alone
    assert np.all(np.isnan(twin.row(h, vp, vs, rho, per, c, nlay=5, Lmax=4)))          # not of the batch's depth
    assert np.all(np.isnan(twin.row(h, vp, vs, rho, per, c, err=1)))                   # the search failed
    for bad_layer in range(5):
        nan_vs = np.array(vs)
        nan_vs[bad_layer] = np.nan
        assert np.all(np.isnan(twin.row(h, vp, nan_vs, rho, per, c)))                  # a NaN model
    for bad in (0.0, np.nan, np.inf, -3.0):                                            # a failed period: its own value only
        cb = c.copy()
        cb[3] = bad
        got = twin.row(h, vp, vs, rho, per, cb)
        assert np.isnan(got[3]) and np.array_equal(np.delete(got, 3), np.delete(good, 3))
    # a model the search cannot solve: every period NaN, the flag set
    ell, c0, err = twin.ellipticity([1., 0.], [np.nan, 6.], [np.nan, 3.5], [2.5, 2.8], per)
    assert err != 0 and np.all(np.isnan(ell))


# ---- layout -------------------------------------------------------------------------------------------------------------
def _parent_layout(swd, rf):
    """RowLayout(swd, rf) as the commit before the ellipticity built it, restated: (slices, ncols, row, tg rows, rf
    offsets, periods, resampled (t, slice, koff))."""
    off, slices = 0, []
    for sp in swd:
        slices.append(slice(off, off + sp.obsx.size))
        off += sp.obsx.size
    rf_off = []
    for r in rf:
        rf_off.append(off)
        slices.append(slice(off, off + r.obsx.size))
        off += r.obsx.size
    ncols, per_off, tg, pers, res = off, 0, [], [], []
    for t, sp in enumerate(swd):
        koff = slices[t].start
        if sp.resample:
            koff = off
            off += sp.periods.size
            res.append((t, slices[t], koff))
        tg.append((sp.iwave, sp.igr, sp.mode, sp.flsph, sp.periods.size, per_off, koff, 0))
        pers.append(sp.periods)
        per_off += sp.periods.size
    return slices, ncols, off, tg, rf_off, np.concatenate(pers) if pers else np.zeros(1), res


def _tg_rows(lay, n):
    return [tuple(getattr(lay.tg[t], f) for f, _ in lay.tg[t]._fields_) for t in range(n)]


def test_layout_without_ellipticity_is_the_parents():
    from bayhunter_amd.layout import RfSpec, RowLayout, SwdSpec
    t201 = np.linspace(-5, 35, 201)
    for swd, rf in (([SwdSpec('rdispph', ec.PER21)], [RfSpec('prf', t201)]),
                    ([SwdSpec('rdispph', ec.PER21), SwdSpec('ldispgr', np.linspace(2, 80, 75), 2, 1)], []),
                    ([], [RfSpec('prf', t201), RfSpec('srf', t201, 2.0, 7.0)]),
                    ([SwdSpec('rdispgr', np.linspace(1, 50, 90)), SwdSpec('rdispph', ec.PER60)], [RfSpec('prf', t201)])):
        lay = RowLayout(swd, rf)
        slices, ncols, row, tg, rf_off, periods, res = _parent_layout(swd, rf)
        assert (lay.slices, lay.ncols, lay.row) == (slices, ncols, row)
        assert len(lay.tg) == max(1, len(swd)) and _tg_rows(lay, len(swd)) == tg
        assert len(lay.rfp) == max(1, len(rf)) and [lay.rfp[i].out_off for i in range(len(rf))] == rf_off
        assert [(lay.rfp[i].p, lay.rfp[i].gauss, lay.rfp[i].nout) for i in range(len(rf))] == \
            [(r.p, r.gauss, r.obsx.size) for r in rf]
        assert lay.periods.tobytes() == np.ascontiguousarray(periods, dtype=np.float64).tobytes()
        assert [(t, sl, k) for t, sl, k, _ in lay.resampled] == res
        assert lay.swd == swd and lay.rf == rf and lay.ell == [] and lay.swd_all == swd and lay.ell_src == []


def test_layout_shares_an_equal_rdispph_target_or_hides_one():
    from bayhunter_amd.layout import EllSpec, RfSpec, RowLayout, SwdSpec
    rf = [RfSpec('prf', np.linspace(-5, 35, 201))]
    e = EllSpec('rellip', ec.PER21)
    assert e.absolute and e.flsph == 0
    # shared: the ellipticity columns follow the receiver function's, nothing is hidden
    shared = RowLayout([SwdSpec('rdispgr', ec.PER21), SwdSpec('rdispph', ec.PER21)], rf, [e])
    assert len(shared.swd_all) == 2 and shared.ell_src == [(1, 21, 21)]
    assert shared.slices[-1] == slice(243, 264) and shared.ell_off == [243] and shared.ncols == shared.row == 264
    # hidden: a group-velocity target, other periods, another mode, another earth, a resampled target do not serve
    for other in (SwdSpec('rdispgr', ec.PER21), SwdSpec('rdispph', ec.PER21 + 1e-9), SwdSpec('rdispph', ec.PER21, 2),
                  SwdSpec('rdispph', ec.PER21, 1, 1), SwdSpec('ldispph', ec.PER21)):
        lay = RowLayout([other], rf, [e])
        assert len(lay.swd) == 1 and len(lay.swd_all) == 2 and len(lay.tg) == 2
        hid = lay.swd_all[1]
        assert (hid.ref, hid.mode, hid.flsph) == ('rdispph', 1, 0) and hid.periods.tobytes() == ec.PER21.tobytes()
        assert lay.slices == [slice(0, 21), slice(21, 222), slice(222, 243)] and lay.ncols == 243
        assert lay.ell_src == [(1, 21, 243)] and lay.row == 264           # the hidden columns lie behind the visible ones
        assert _tg_rows(lay, 2)[1] == (2, 0, 1, 0, 21, 21, 243, 0)
        assert lay.periods.size == 42
    # a resampled visible target keeps its scratch columns; the hidden target's come first, behind ncols
    lay = RowLayout([SwdSpec('rdispph', np.linspace(1, 50, 90))], [], [EllSpec('rellip', ec.PER60, 1, False)])
    assert lay.ncols == 150 and lay.row == 150 + 60 + 60 and len(lay.resampled) == 1
    assert sorted([lay.tg[0].out_off, lay.tg[1].out_off]) == [150, 210] and lay.ell_src[0][2] == lay.tg[1].out_off
    # two ellipticity targets on the same periods share one hidden target
    lay = RowLayout([], [], [EllSpec('rellip', ec.PER21), EllSpec('rellip', ec.PER21, absolute=False)])
    assert len(lay.swd_all) == 1 and lay.ell_src == [(0, 0, 42), (0, 0, 42)] and lay.row == 63


def test_more_than_60_periods_are_refused():
    from bayhunter_amd import plugins, targets
    from bayhunter_amd.layout import EllSpec
    x = np.linspace(1, 40, 61)
    with pytest.raises(ValueError):
        EllSpec('rellip', x)
    with pytest.raises(ValueError):
        plugins.RayleighEllipticity(x)
    with pytest.raises(ValueError):
        targets.RayleighEllipticity(x, np.ones(61))
    with pytest.raises(ReferenceError):
        EllSpec('rdispph', x[:10])
    assert EllSpec('rellip', x[:60]).periods.size == 60


def test_target_type_and_batch_layout():
    from bayhunter_amd import plugins, targets
    t = targets.RayleighEllipticity(ec.PER21, np.ones(21))
    assert t.ref == 'rellip' and t.noiseref == 'swd' and isinstance(t.moddata.plugin, plugins.RayleighEllipticity)
    p = t.moddata.plugin
    assert p.modelparams == {'flsph': 0, 'absolute': True}
    p.set_modelparams(flsph=1, absolute=False)
    assert p.modelparams == {'flsph': 1, 'absolute': False}
    joint = targets.JointTarget([targets.RayleighDispersionPhase(ec.PER21, np.ones(21)), t])
    with pytest.raises(TypeError):                            # the evaluation plan does not know the target yet
        joint.batch_layout()


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_before_it_touches_a_device(lib):
    from bayhunter_amd import _lib
    p = C.c_void_p(64)            # never dereferenced: every call below is refused first

    def batch(nper=21, c_stride=21, err_stride=1, out_stride=21, null=None, Lmax=10, mstride=10):
        a = [4, Lmax, mstride, p, p, p, p, p, nper, p, 0, p, c_stride, p, err_stride, 1, p, out_stride, None]
        if null is not None:
            a[null] = None
        return lib.bh_ell_batch(*a)
    for kw in (dict(nper=0), dict(nper=_lib.MAX_PERIODS + 1), dict(c_stride=20), dict(out_stride=20), dict(err_stride=0),
               dict(Lmax=0), dict(Lmax=_lib.MAX_LAYERS + 1), dict(mstride=9)) + tuple(dict(null=i) for i in
                                                                                      (3, 4, 5, 6, 7, 9, 11, 13, 16)):
        assert batch(**kw) == _lib.BH_ERR_ARG, kw
        assert lib.bh_last_error()
    f = np.ones(4, dtype=np.float32)
    t, out, err = np.linspace(1, 10, 61), np.zeros(61), C.c_int(0)

    def single(n=4, kmax=21, null=None):
        a = [f.ctypes.data] * 4 + [n, 0, kmax, t.ctypes.data, 1, out.ctypes.data, C.byref(err)]
        if null is not None:
            a[null] = None
        return lib.bh_ellipticity(*a)
    for kw in (dict(kmax=0), dict(kmax=61), dict(n=0), dict(n=101), dict(null=0), dict(null=3), dict(null=7), dict(null=9),
               dict(null=10)):
        assert single(**kw) == _lib.BH_ERR_ARG, kw
