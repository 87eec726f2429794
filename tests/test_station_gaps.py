"""Stations with data gaps (StationPool(missing='mask'), bh_likelihood_sets_gaps, bh_eval_set_gaps), CPU tier.

A target with gaps is valued as the reference's Valuation (src/Targets.py:99-183) values it when the missing lines
have been deleted from the data file.  Checked here without a GPU:
  * the host replay of like_gaps_kernel's staging and closed forms (tests/hostsim/like_gaps_sim.cpp, the functions of
    bayhunter_amd/csrc/like_core.h) against likelihood_hp.evaluate on the COMPACTED arrays, inside that module's own
    bounds for n' samples; bit for bit against the unmasked replay of the compacted arrays; a full mask bit for bit
    against the unmasked replay;
  * the tables a StationPool hands to its evaluation plans, the host-side valuation, every refusal, and a pool with
    gaps on CPU evaluators."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import likelihood_hp as hp
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
from chain_scenario import CASES, oracle_evaluator  # noqa: E402
from station_scenario import make_stations, station_evaluator  # noqa: E402

DATA = os.path.join(GOLDEN, 'tutorial_observed')
KEYS = ('models', 'likes', 'misfits', 'noise', 'vpvs', 'iter')
SIZES = (3, 64, 65, 129)
MASKS = ('first', 'last', 'both', 'alternate', 'one', 'full')


def mask_of(kind, n):
    m = np.ones(n, dtype=np.uint8)
    if kind in ('first', 'both'):
        m[0] = 0
    if kind in ('last', 'both'):
        m[-1] = 0
    if kind == 'alternate':
        m[1::2] = 0
    if kind == 'one':
        m[:] = 0
        m[n // 2] = 1
    return m


# ---- host replay ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gaps_sim():
    """tests/hostsim/like_gaps_sim.cpp with g++ and glibc math (the flags of conftest's hostsim build)."""
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so, src = os.path.join(d, 'liblike_gaps_sim.so'), os.path.join(d, 'like_gaps_sim.cpp')
    deps = [src] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', f) for f in ('bh_common.h', 'like_core.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-DBH_HOSTSIM_GLIBC_MATH',
                        '-o', so, src], check=True)
    hs = C.CDLL(so)
    vp_, i_ = C.c_void_p, C.c_int
    hs.hs_like_gaps.restype = i_
    hs.hs_like_gaps.argtypes = [i_, i_, vp_, vp_, vp_, i_, i_, vp_, vp_, i_, vp_, vp_, vp_, vp_, vp_, vp_, vp_]
    return hs


def replay(hs, targets, out, yobs, scale, logdet, noise, obs_id=None, present=None):
    """targets: likelihood_hp.Target; yobs, scale [nsets, stride]; logdet [nsets, T] -> (rc, logL, misfits, bad)."""
    M, T = out.shape[0], len(targets)
    tg = np.ascontiguousarray([[t.n, t.off, t.cov] for t in targets], dtype=np.int32)
    extra = np.ascontiguousarray([t.logdet_extra for t in targets], dtype=np.float64)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (out, yobs, scale, logdet, noise)]
    oid = None if obs_id is None else np.ascontiguousarray(obs_id, dtype=np.int32)
    pres = None if present is None else np.ascontiguousarray(present, dtype=np.uint8)
    logL, mis, bad = np.full(M, np.nan), np.full((M, T + 1), np.nan), np.full(2, -1, dtype=np.int32)
    rc = hs.hs_like_gaps(M, T, tg.ctypes.data, extra.ctypes.data, arrs[0].ctypes.data, out.shape[1], arrs[1].shape[0],
                         None if oid is None else oid.ctypes.data, arrs[1].ctypes.data, arrs[1].shape[1],
                         arrs[2].ctypes.data, arrs[3].ctypes.data, arrs[4].ctypes.data,
                         None if pres is None else pres.ctypes.data, logL.ctypes.data, mis.ctypes.data, bad.ctypes.data)
    return rc, logL, mis, bad


def draw(cov, n, M, seed, off=2, pad=3):
    """One target of n samples at column `off` of a row with `pad` unused columns behind it, one observation set."""
    rs = np.random.RandomState(seed)
    stride = off + n + pad
    yobs = rs.standard_normal((1, stride))
    out = yobs[0] + rs.standard_normal((M, stride)) * 10.0 ** rs.uniform(-3, 0, M)[:, None]
    noise = np.stack([rs.uniform(-0.95, 0.95, M), rs.uniform(0.005, 2.0, M)], axis=1)
    noise[0, 0] = 0.999999                          # likelihood_hp.CORRS' edge
    yerr = rs.uniform(0.01, 0.04, stride)
    return dict(cov=cov, n=n, off=off, stride=stride, out=out, yobs=yobs, noise=noise, yerr=yerr)


def tables(k, mask):
    """The caller's tables for the masked call: scaled errors and their log-product over the kept samples."""
    sl = slice(k['off'], k['off'] + k['n'])
    present = np.ones((1, k['stride']), dtype=np.uint8)
    present[0, sl] = mask
    keep = np.nonzero(mask)[0]
    scale = np.ones((1, k['stride']))
    se = k['yerr'][sl][keep] / k['yerr'][sl][keep].min()
    scale[0, k['off'] + keep] = se
    logdet = np.array([[np.log(np.prod(se))]])
    return present, keep, se, scale, logdet


def compacted(k, keep, se):
    """The arrays of a call on the shortened data file: one target of n' samples at column 0."""
    cols = k['off'] + keep
    tg = hp.Target(len(keep), 0, k['cov'], 0, float(np.log(np.prod(se))) if k['cov'] == hp.COV_NOCORR_SCALED else 0.0)
    return tg, np.ascontiguousarray(k['out'][:, cols]), np.ascontiguousarray(k['yobs'][:, cols])


@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('cov', [hp.COV_NOCORR, hp.COV_NOCORR_SCALED, hp.COV_EXP])
def test_host_replay_of_the_masked_forms_is_the_compacted_call(gaps_sim, cov, n, kind):
    """Masked replay = extended-precision evaluation of the compacted arrays inside likelihood_hp's bounds for n'
    samples, = unmasked replay of the compacted arrays bit for bit; a full mask = the unmasked replay bit for bit."""
    M = 9
    k = draw(cov, n, M, seed=1000 * cov + 10 * n + MASKS.index(kind))
    mask = mask_of(kind, n)
    present, keep, se, scale, logdet = tables(k, mask)
    full = hp.Target(n, k['off'], cov, 0, float(logdet[0, 0]) if cov == hp.COV_NOCORR_SCALED else 0.0)
    rc, logL, mis, _ = replay(gaps_sim, [full], k['out'], k['yobs'], scale, logdet, k['noise'], present=present)
    assert rc == 0 and np.isfinite(logL).all() and np.isfinite(mis).all()
    tg, out_c, yobs_c = compacted(k, keep, se)
    assert tg.n == {'first': n - 1, 'last': n - 1, 'both': n - 2, 'alternate': (n + 1) // 2, 'one': 1, 'full': n}[kind]
    ref = hp.evaluate(out_c, yobs_c, k['noise'], se, [tg])
    case = dict(rows=np.arange(M), poisoned=[], case=dict(name='%s_n%d_%s' % (hp.FORM_NAMES[cov], n, kind)))
    rl, rm, msg = hp.judge(case, logL, mis, ref=ref)
    print('HP-RATIO host-gaps %s logL=%.3f misfit=%.3f' % (case['case']['name'], rl, rm))
    assert msg is None, msg
    rc, logL_c, mis_c, _ = replay(gaps_sim, [tg], out_c, yobs_c, se[None, :], logdet, k['noise'])
    assert rc == 0 and logL.tobytes() == logL_c.tobytes() and mis.tobytes() == mis_c.tobytes()
    if kind == 'full':
        rc, logL_u, mis_u, _ = replay(gaps_sim, [full], k['out'], k['yobs'], scale, logdet, k['noise'])
        assert rc == 0 and logL.tobytes() == logL_u.tobytes() and mis.tobytes() == mis_u.tobytes()
    else:
        rc, logL_u, _, _ = replay(gaps_sim, [full], k['out'], k['yobs'], scale, logdet, k['noise'])
        assert not np.array_equal(logL, logL_u)                      # the mask is not ignored


@pytest.mark.parametrize('n', SIZES)
def test_host_tables_refuse_a_dense_target_with_a_gap_and_an_empty_target(gaps_sim, n):
    """The fourth covariance code: BH_COV_GAUSS cannot have gaps (code 1, naming set and target), with a full mask it
    passes the table builder; a target without a kept sample is code 2 whatever its covariance."""
    k = draw(hp.COV_NOCORR, n, 2, seed=n)
    other = hp.Target(2, 0, hp.COV_NOCORR, 0, 0.0)
    yobs, ones = np.repeat(k['yobs'], 3, axis=0), np.ones((3, k['stride']))
    logdet = np.zeros((3, 2))
    for kind in MASKS[:-1]:
        present = np.ones((3, k['stride']), dtype=np.uint8)
        present[2, k['off']:k['off'] + n] = mask_of(kind, n)
        dense = hp.Target(n, k['off'], hp.COV_GAUSS, 0, 0.0)
        rc, _, _, bad = replay(gaps_sim, [other, dense], k['out'], yobs, ones, logdet, k['noise'], present=present)
        assert rc == 1 and list(bad) == [2, 1], kind
    for cov in (hp.COV_NOCORR, hp.COV_NOCORR_SCALED, hp.COV_EXP):
        present = np.ones((3, k['stride']), dtype=np.uint8)
        present[1, k['off']:k['off'] + n] = 0
        rc, _, _, bad = replay(gaps_sim, [other, hp.Target(n, k['off'], cov, 0, 0.0)], k['out'], yobs, ones, logdet,
                               k['noise'], present=present)
        assert rc == 2 and list(bad) == [1, 1]


def test_host_replay_with_several_sets_and_targets(gaps_sim):
    """Three sets with their own masks, rows in mixed order, three targets in one row: every row equals the
    single-target compacted replay of its own set, so neither the neighbours' sets nor the other targets leak in."""
    rs = np.random.RandomState(5)
    ns, covs, offs = (65, 21, 129), (hp.COV_EXP, hp.COV_NOCORR_SCALED, hp.COV_NOCORR), (1, 70, 95)
    stride, nsets, M = 230, 3, 11
    yobs = rs.standard_normal((nsets, stride))
    obs_id = rs.randint(0, nsets, M).astype(np.int32)
    obs_id[:3] = [0, 1, 2]
    out = yobs[obs_id] + 0.1 * rs.standard_normal((M, stride))
    noise = np.tile(np.stack([rs.uniform(-0.9, 0.9, M), rs.uniform(0.01, 1.0, M)], axis=1), (1, 3))
    yerr = rs.uniform(0.01, 0.04, (nsets, stride))
    present = np.ones((nsets, stride), dtype=np.uint8)
    for t, (n, off) in enumerate(zip(ns, offs)):
        present[1, off:off + n] = mask_of(('both', 'alternate', 'first')[t], n)
        present[2, off:off + n] = rs.uniform(size=n) > 0.3
    present[2, offs[0]:offs[0] + ns[0]] = mask_of('one', ns[0])
    scale, logdet = np.ones((nsets, stride)), np.zeros((nsets, 3))
    for s in range(nsets):
        keep = offs[1] + np.nonzero(present[s, offs[1]:offs[1] + ns[1]])[0]
        scale[s, keep] = yerr[s, keep] / yerr[s, keep].min()
        logdet[s, 1] = np.log(np.prod(scale[s, keep]))
    targets = [hp.Target(n, off, cov, 0, 0.0) for n, off, cov in zip(ns, offs, covs)]
    rc, logL, mis, _ = replay(gaps_sim, targets, out, yobs, scale, logdet, noise, obs_id, present)
    assert rc == 0
    want_l, want_m = np.zeros(M), np.zeros((M, 4))
    for b in range(M):
        s = obs_id[b]
        for t, (n, off, cov) in enumerate(zip(ns, offs, covs)):
            cols = off + np.nonzero(present[s, off:off + n])[0]
            rc, l, m, _ = replay(gaps_sim, [hp.Target(len(cols), 0, cov, 0, 0.0)], out[b:b + 1, cols], yobs[s:s + 1, cols],
                                 scale[s:s + 1, cols], logdet[s:s + 1, t:t + 1], noise[b:b + 1, 2 * t:2 * t + 2])
            assert rc == 0
            want_l[b] += l[0]
            want_m[b, t] = m[0, 0]
            want_m[b, 3] += m[0, 0]
    assert logL.tobytes() == want_l.tobytes() and mis.tobytes() == want_m.tobytes()


# ---- the Python layer -----------------------------------------------------------------------------------------
def _params(burnin=60, main=40):
    case = CASES['tutorial']
    return dict(case['initparams'], iter_burnin=burnin, iter_main=main), case['priors']


def _covariances(stations, corrfix=(True, False), corr=(0.0, 0.5)):
    for joint in stations:
        joint.set_target_covariance(list(corrfix), list(corr), 1e-5)


def test_observation_tables_renormalise_the_scale_over_the_kept_samples():
    """A gap at the sample that holds yerr.min(): scaled_err = yerr / min over the KEPT samples, its log-product over
    them, 1 and a finite yobs at the gap, present = 0 there; the station without gaps keeps its numbers."""
    from bayhunter_amd import _lib
    from bayhunter_amd.stations import find_gaps, observation_tables
    st = make_stations(DATA, 2, yerr=True)
    _covariances(st)
    assert st[1].targets[0].covmodel == _lib.COV_NOCORR_SCALED and st[1].targets[1].covmodel == _lib.COV_EXP
    before = observation_tables(st)
    tg = st[1].targets[0]
    lo = int(np.argmin(tg.obsdata.yerr))
    y = tg.obsdata.y.copy()
    y[lo] = np.nan
    y[-1] = np.inf
    tg.obsdata.y = y
    rf = st[1].targets[1]
    ry = rf.obsdata.y.copy()
    ry[:5] = np.nan
    rf.obsdata.y = ry
    assert find_gaps(['a', 'b'], st, 'mask') == 7
    yobs, scale, logdet, present = observation_tables(st, present=True)
    assert np.isfinite(yobs).all() and np.isfinite(scale).all() and present.dtype == np.uint8
    bl = st[1].batch_layout()
    d0, d1 = bl['desc'][0], bl['desc'][1]
    keep = np.ones(d0.n, dtype=bool)
    keep[[lo, d0.n - 1]] = False
    assert np.array_equal(present[1, d0.off:d0.off + d0.n], keep) and present[0].all()
    assert not present[1, d1.off:d1.off + 5].any() and present[1, d1.off + 5:d1.off + d1.n].all()
    want = tg.obsdata.yerr[keep] / tg.obsdata.yerr[keep].min()
    got = scale[1, d0.off:d0.off + d0.n]
    assert np.array_equal(got[keep], want) and want.min() == 1.0 and np.all(got[~keep] == 1.0)
    assert not np.array_equal(got[keep], (tg.obsdata.yerr / tg.obsdata.yerr.min())[keep])      # renormalised
    assert logdet[1, 0] == np.log(np.prod(want))
    assert np.array_equal(yobs[1, d0.off:d0.off + d0.n][keep], y[keep])
    for a, b in zip(before, (yobs, scale, logdet)):
        assert np.array_equal(a[0], b[0])
    assert observation_tables(st)[0].shape == yobs.shape                   # the three-table form is unchanged
    st2 = make_stations(DATA, 2, yerr=True)
    _covariances(st2)
    assert find_gaps(['a', 'b'], st2, 'mask') == 0 and observation_tables(st2, present=True)[3] is None


def test_host_valuation_of_a_target_with_gaps_is_the_reference_on_the_shortened_data():
    """SingleTarget.quadratic_form / calc_misfit over the kept samples against the reference's own recipe on the
    shortened arrays: get_covariance_*(size = n') and get_likelihood (src/Targets.py:105-183)."""
    from bayhunter_amd.stations import find_gaps
    from bayhunter_amd.targets import LOG_2PI, Valuation
    st = make_stations(DATA, 1, yerr=True)
    rs = np.random.RandomState(3)
    for corrfix, corr in (((True, False), (0.0, 0.5)), ((False, True), (0.3, 0.0))):
        _covariances(st, corrfix, corr)
        for tg, c in zip(st[0].targets, corr):
            y = np.array(tg.obsdata.y, dtype=np.float64)
            y[~np.isfinite(y)] = 0.1
            miss = rs.choice(y.size, y.size // 3, replace=False)
            ymod = y + 0.05 * rs.standard_normal(y.size)
            y[miss] = np.nan
            tg.obsdata.y = y
            find_gaps(['a'], st, 'mask')
            keep = tg.present
            assert keep is not None and keep.sum() == y.size - miss.size
            sigma = 0.07
            madist, logdet = tg.quadratic_form(tg.kept(ymod - y), c, sigma)
            got = -0.5 * (keep.sum() * LOG_2PI + logdet) - madist / 2.
            v = Valuation()
            kw = dict(sigma=sigma, size=int(keep.sum()), yerr=tg.obsdata.yerr[keep], corr=c)
            c_inv, logc_det = getattr(v, tg.get_covariance.__name__)(**kw)
            want = v.get_likelihood(y[keep], ymod[keep], c_inv, logc_det)
            assert abs(got - want) <= 1e-9 * abs(want), (tg.ref, got, want)
            tg.moddata.x, tg.moddata.y = tg.obsdata.x, ymod
            tg.calc_misfit()
            assert tg.valuation.misfit == v.get_rms(y[keep], ymod[keep])


def _build(stations, **kw):
    from bayhunter_amd.stations import StationPool
    ip, priors = _params()
    return StationPool(stations, ip, priors, chains_per_station=2, random_seeds=list(range(len(stations))),
                       evaluator=lambda p, n, z, s: None, **kw)


def _with_nan(target=0, sample=3, station=1, field='y', n=2, **kw):
    st = make_stations(DATA, n, **kw)
    tg = st[station].targets[target]
    a = np.array(getattr(tg.obsdata, field), dtype=np.float64)
    a[sample] = np.nan if field == 'y' else np.inf
    setattr(tg.obsdata, field, a)
    return st


def test_missing_refuse_is_the_default_and_names_station_target_and_sample():
    with pytest.raises(ValueError, match=r"station 'st001', target 0 \(rdispph\): y is not finite at sample 3 "):
        _build(_with_nan())
    with pytest.raises(ValueError, match=r"station 'st000', target 1 \(prf\): y is not finite at sample 0 "):
        _build(_with_nan(target=1, sample=0, station=0), missing='refuse')
    priors = dict(CASES['tutorial']['priors'], swdnoise_corr=0.0)          # corr fixed at 0 + yerr: the scaled model
    from bayhunter_amd.stations import StationPool
    ip, _ = _params()
    with pytest.raises(ValueError, match=r"station 'st001', target 0 \(rdispph\): yerr is not finite at sample 4 "):
        StationPool(_with_nan(field='yerr', sample=4, yerr=True), ip, priors, chains_per_station=2, random_seeds=[1, 2],
                    evaluator=lambda p, n, z, s: None)
    with pytest.raises(ValueError, match="missing='drop'"):
        _build(make_stations(DATA, 2), missing='drop')
    _build(make_stations(DATA, 2)).close()                                # clean data: as before


def test_mask_refuses_a_dense_target_with_a_gap_and_an_empty_target():
    from bayhunter_amd import _lib
    from bayhunter_amd.stations import StationPool
    ip, _ = _params()
    priors = dict(CASES['tutorial']['priors'], rfnoise_corr=0.9)           # fixed, non-zero: the dense Gaussian model
    with pytest.raises(ValueError, match=r"station 'st001', target 1 \(prf\): 1 samples are missing.*dense Gaussian"):
        StationPool(_with_nan(target=1), ip, priors, chains_per_station=2, random_seeds=[1, 2],
                    evaluator=lambda p, n, z, s: None, missing='mask')
    pool = StationPool(_with_nan(target=0), ip, priors, chains_per_station=2, random_seeds=[1, 2],
                       evaluator=lambda p, n, z, s: None, missing='mask')   # the gap is in the other target
    assert pool.ngaps == 1 and pool.stations[1].targets[1].covmodel == _lib.COV_GAUSS
    pool.close()
    st = make_stations(DATA, 2)
    st[0].targets[0].obsdata.y = np.full(st[0].targets[0].obsdata.y.size, np.nan)
    with pytest.raises(ValueError, match=r"station 'st000', target 0 \(rdispph\): no sample is left"):
        _build(st, missing='mask')
    pool = _build(_with_nan(), missing='mask')
    assert pool.missing == 'mask' and pool.ngaps == 1
    assert pool.stations[0].targets[0].present is None and not pool.stations[1].targets[0].present[3]
    pool.close()


def test_a_layout_with_gaps_does_not_run_without_them():
    """JointTarget.evaluate_batch has no table of gaps to give: refused rather than run on the placeholders."""
    pool = _build(_with_nan(), missing='mask')
    with pytest.raises(ValueError, match="data gaps"):
        pool.stations[1]._build_batch()
    pool.close()


@pytest.fixture(scope='module')
def gap_stations_pool(oracle):
    """3 stations x 3 chains on the oracle's CPU evaluators, gaps at stations 1 and 2."""
    from bayhunter_amd.stations import StationPool
    ip, priors = _params()
    priors = dict(priors, rfnoise_corr=(0.5, 0.95))        # a free correlation: the exponential law, which may have gaps

    def stations():
        st = make_stations(DATA, 3, oracle=oracle, yerr=True)
        for s, (a, b) in ((1, (0, 4)), (2, (15, 21))):
            y = st[s].targets[0].obsdata.y.copy()
            y[a:b] = np.nan
            st[s].targets[0].obsdata.y = y
        ry = st[2].targets[1].obsdata.y.copy()
        ry[::7] = np.nan
        st[2].targets[1].obsdata.y = ry
        return st

    def pool(st, seeds):
        ev = station_evaluator([oracle_evaluator(j) for j in st])
        return StationPool(st, ip, priors, chains_per_station=3, random_seeds=seeds, evaluator=ev, nmodels=101,
                           missing='mask').run()
    return stations, pool, pool(stations(), [7, 8, 9])


def test_a_pool_with_gaps_runs_on_cpu_evaluators(oracle, gap_stations_pool):
    """Every station of the pool is the one-station StationPool(missing='mask') of it, array for array; the station
    without gaps is its plain ChainPool; the likelihoods are finite and differ from those of the complete data."""
    from bayhunter_amd.chains import ChainPool
    stations, make, pool = gap_stations_pool
    assert pool.ngaps == 4 + 6 + len(range(0, pool.stations[2].targets[1].obsdata.y.size, 7))
    assert np.nanmin(pool.pool.likes) > -1e14                              # no NaN likelihood was ever accepted
    for s in range(3):
        single = make([stations()[s]], [7 + s])
        for k in KEYS:
            assert np.array_equal(getattr(pool.station(s), k), getattr(single.station(0), k), equal_nan=True), (s, k)
        single.close()
    ip, priors = _params()
    priors = dict(priors, rfnoise_corr=(0.5, 0.95))
    joint = make_stations(DATA, 1, oracle=oracle, yerr=True)[0]
    plain = ChainPool(joint, ip, priors, random_seed=7, nchains=3, evaluator=oracle_evaluator(joint), nmodels=101).run()
    for k in KEYS:
        assert np.array_equal(getattr(pool.station(0), k), getattr(plain, k), equal_nan=True), k
    complete = make_stations(DATA, 3, oracle=oracle, yerr=True)[1]
    other = ChainPool(complete, ip, priors, random_seed=8, nchains=3, evaluator=oracle_evaluator(complete), nmodels=101).run()
    assert not np.array_equal(pool.station(1).likes, other.likes, equal_nan=True)
    for p in (plain, other):
        p.close()


# ---- the C ABI, before any device call --------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared(lib):
    from bayhunter_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read().replace('int  ', 'int ')
    for name in ('bh_likelihood_sets_gaps', 'bh_eval_set_gaps'):
        assert name in _lib.EXPORTS and hasattr(lib, name) and ('int %s(' % name) in header
    assert 'size_t bh_likelihood_gaps_workspace_bytes(' in header
    assert lib.bh_likelihood_gaps_workspace_bytes(3, 100, 4) == (3 * 100 + 3 * 4) * 4
    assert lib.bh_likelihood_gaps_workspace_bytes(0, 100, 4) == 0


def test_likelihood_sets_gaps_validates_arguments_without_gpu(lib):
    """Every refusal is decided on the host, before the first device call: the sets' own checks, the workspace, a
    BH_COV_GAUSS target with a gap and a target without a kept sample, naming set and target."""
    from bayhunter_amd import _lib
    stride, nsets = 40, 3
    targets = (_lib.LikeTarget * 3)(_lib.LikeTarget(10, 0, _lib.COV_EXP, 0, 0.0),
                                    _lib.LikeTarget(12, 10, _lib.COV_GAUSS, 0, 0.0),
                                    _lib.LikeTarget(15, 24, _lib.COV_NOCORR, 0, 0.0))
    need = lib.bh_likelihood_gaps_workspace_bytes(nsets, stride, 3)

    def call(present, nsets=nsets, ws=1, ws_bytes=need, obs_id=1, B=4, set_stride=stride):
        p = None if present is None else np.ascontiguousarray(present, dtype=np.uint8)
        return lib.bh_likelihood_sets_gaps(3, B, 3, targets, 1, stride, None, 0, nsets, obs_id, 1, set_stride, None, None, 1,
                                           1, 1, 1, None, 0, None if p is None else p.ctypes.data, ws, ws_bytes, None)
    ones = np.ones((nsets, stride), dtype=np.uint8)
    assert call(ones, B=0) == _lib.BH_OK                                           # nothing to do
    assert call(ones, nsets=0) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert call(ones, obs_id=None) == _lib.BH_ERR_ARG and b'obs_id' in lib.bh_last_error()
    assert call(ones, set_stride=30) == _lib.BH_ERR_ARG and b'set_stride' in lib.bh_last_error()
    assert call(ones, ws=None) == _lib.BH_ERR_WORKSPACE and b'gaps_workspace' in lib.bh_last_error()
    assert call(ones, ws_bytes=need - 1) == _lib.BH_ERR_WORKSPACE and b'gaps_workspace' in lib.bh_last_error()
    p = ones.copy()
    p[2, 15] = 0
    assert call(p) == _lib.BH_ERR_ARG
    assert b'set 2, target 1' in lib.bh_last_error() and b'BH_COV_GAUSS' in lib.bh_last_error()
    p = ones.copy()
    p[1, 24:39] = 0
    assert call(p) == _lib.BH_ERR_ARG and b'set 1, target 2' in lib.bh_last_error() and b'no sample' in lib.bh_last_error()
    p = ones.copy()
    p[0, :10] = 0
    p[0, 22:24] = 0                                                               # (columns of no target: not read)
    assert call(p) == _lib.BH_ERR_ARG and b'set 0, target 0' in lib.bh_last_error()


def test_eval_set_gaps_validates_arguments_without_gpu(lib):
    from bayhunter_amd import _lib
    p = np.ones((3, 50), dtype=np.uint8)
    assert lib.bh_eval_set_gaps(None, 0, p.ctypes.data) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert lib.bh_eval_set_gaps(None, 3, None) == _lib.BH_ERR_ARG and b'NULL' in lib.bh_last_error()
    assert lib.bh_eval_set_gaps(None, 3, p.ctypes.data) == _lib.BH_ERR_ARG and b'plan is NULL' in lib.bh_last_error()
