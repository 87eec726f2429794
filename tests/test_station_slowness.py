"""Per-station receiver-function slowness (StationPool(per_station=('p',)), bh_rf_batch_sets, bh_eval_set_rf_slowness),
CPU tier: the pool with every station's own ray parameter against single-station pools (oracle evaluators), the
refusals, a host replay of the per-row form of rf_kernel against the uniform form, and the argument checks of the
two C entry points that are decided before any device call.

Every comparison is exact: a row computed at its station's p is the row a pool of that station alone computes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
from chain_scenario import CASES, OraclePlugin, oracle_evaluator  # noqa: E402
from station_scenario import make_stations, station_evaluator  # noqa: E402

DATA = os.path.join(GOLDEN, 'tutorial_observed')
KEYS = ('models', 'likes', 'misfits', 'noise', 'vpvs', 'iter')
P = (5.2, 6.4, 7.9)
BURNIN, MAIN = 90, 50


class SlownessOraclePlugin(OraclePlugin):
    """The oracle's receiver function at this station's own ray parameter, which it carries like RFminiModRF does."""

    def __init__(self, oracle, x, kind, p):
        OraclePlugin.__init__(self, oracle, x, kind)
        self.modelparams = {'p': float(p)}

    def run_model(self, h, vp, vs, rho, **kw):
        return self.obsx, self.oracle.rf_model(h, vp, vs, rho, p=self.modelparams['p'], nout=self.obsx.size,
                                               waveno=self.args[0])


def _stations(oracle, ps, same_data=False):
    if same_data:
        st = [make_stations(DATA, 1, oracle=oracle, yerr=True)[0] for _ in ps]
    else:
        st = make_stations(DATA, len(ps), oracle=oracle, yerr=True)
    for joint, p in zip(st, ps):
        rf = joint.targets[1]
        assert rf.noiseref == 'rf'
        rf.update_plugin(SlownessOraclePlugin(oracle, rf.obsdata.x, 'prf', p))
    return st


def _params():
    case = CASES['tutorial']
    return dict(case['initparams'], iter_burnin=BURNIN, iter_main=MAIN), case['priors']


def _pool(oracle, ps, seeds, same_data=False, **kw):
    from bayhunter_amd.stations import StationPool
    ip, priors = _params()
    st = _stations(oracle, ps, same_data)
    ev = station_evaluator([oracle_evaluator(j) for j in st])
    return StationPool(st, ip, priors, chains_per_station=3, random_seeds=seeds, evaluator=ev,
                       nmodels=BURNIN + MAIN + 1, **kw)


@pytest.fixture(scope='module')
def singles(oracle):
    from bayhunter_amd.chains import ChainPool
    ip, priors = _params()
    return [ChainPool(joint, ip, priors, random_seed=7 + s, nchains=3, evaluator=oracle_evaluator(joint),
                      nmodels=BURNIN + MAIN + 1).run() for s, joint in enumerate(_stations(oracle, P))]


@pytest.mark.parametrize('kw', [dict(), dict(lookahead=4), dict(groups=2)], ids=['plain', 'lookahead', 'groups'])
def test_stations_with_their_own_slowness_are_their_single_pools(oracle, singles, kw):
    """3 stations x 3 chains of the tutorial set-up, p = 5.2 / 6.4 / 7.9 s/deg: every station's chains are the chains
    of a ChainPool of that station alone, array for array."""
    pool = _pool(oracle, P, [7, 8, 9], per_station=('p',), **kw).run()
    assert pool.per_station == ('p',) and pool.nchains == 9
    for s in range(3):
        view, single = pool.station(s), singles[s]
        for k in KEYS:
            assert np.array_equal(getattr(view, k), getattr(single, k), equal_nan=True), (s, k)
        for a, b in zip(view.counters(), single.counters()):
            assert np.array_equal(a, b)
        assert view.targets.targets[1].moddata.plugin.modelparams['p'] == P[s]      # what datafits() / save() use
    pool.close()


def test_same_data_and_seed_but_other_slowness_give_other_likelihoods(oracle):
    pool = _pool(oracle, (5.2, 7.9), [5, 5], same_data=True, per_station=('p',)).run()
    a, b = pool.station(0), pool.station(1)
    assert np.array_equal(a.seeds, b.seeds)
    assert np.array_equal(a.models[:, 0], b.models[:, 0], equal_nan=True)            # same initial models
    assert not np.array_equal(a.likes[:, 0], b.likes[:, 0])
    assert not np.array_equal(a.likes, b.likes, equal_nan=True)
    same = _pool(oracle, (6.4, 6.4), [5, 5], same_data=True, per_station=('p',)).run()
    assert np.array_equal(same.station(0).likes, same.station(1).likes, equal_nan=True)


def test_refusals_with_and_without_the_opt_in():
    from bayhunter_amd.stations import StationPool, check_stations
    ip, priors = _params()

    def build(stations, **kw):
        return StationPool(stations, ip, priors, chains_per_station=2, random_seeds=list(range(len(stations))),
                           evaluator=lambda p, n, z, s: None, **kw)

    def differing(key, val):
        st = make_stations(DATA, 2, yerr=True)
        st[1].targets[1].moddata.plugin.set_modelparams(**{key: val})
        return st
    with pytest.raises(ValueError, match=r"per_station='gauss'.*'p'"):
        build(make_stations(DATA, 2, yerr=True), per_station=('gauss',))
    with pytest.raises(ValueError, match=r"station 'st001'.*target 1.*'p'.*per-station plugin parameters are not supported"):
        build(differing('p', 7.0))                                   # no opt-in: the message it always had
    with pytest.raises(ValueError, match=r"station 'st001'.*target 1.*'gauss'"):
        build(differing('gauss', 2.0), per_station=('p',))
    st = differing('p', 7.0)
    st[1].targets[0].moddata.plugin.set_modelparams(mode=2)           # the opt-in is about receiver functions only
    with pytest.raises(ValueError, match=r"station 'st001'.*target 0.*'mode'"):
        build(st, per_station=('p',))
    pool = build(differing('p', 7.0), per_station=('p',))
    assert pool.per_station == ('p',)
    pool.close()
    build(differing('p', 7.0), per_station='p').close()              # a single name
    st = differing('p', 7.0)
    for j in st:
        j.set_target_covariance([True, True], [0.0, 0.9], 1e-5)
    check_stations(['a', 'b'], st, ('p',))
    with pytest.raises(ValueError, match="'p'"):
        check_stations(['a', 'b'], st)
    from bayhunter_amd.stations import rf_slowness_table
    assert np.array_equal(rf_slowness_table(st), [[6.4], [7.0]])


# ---- host replay of the per-row form ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sets_sim():
    """tests/hostsim/rf_sets_sim.cpp with g++ and glibc math (the flags of conftest's hostsim build)."""
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so, src = os.path.join(d, 'librf_sets_sim.so'), os.path.join(d, 'rf_sets_sim.cpp')
    deps = [src] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', f) for f in ('bh_common.h', 'bh_math.h', 'rf_core.h', 'rf_host.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-DBH_HOSTSIM_GLIBC_MATH',
                        '-o', so, src], check=True)
    hs = C.CDLL(so)
    hs.hs_rf_sets_spectra.restype = hs.hs_rf_spectrum.restype = C.c_int
    vp_, i_, d_ = C.c_void_p, C.c_int, C.c_double
    hs.hs_rf_sets_spectra.argtypes = [i_, i_, vp_, vp_, vp_, vp_, vp_, i_, vp_, vp_, d_, i_, d_, d_, d_, i_, i_, vp_, vp_]
    hs.hs_rf_spectrum.argtypes = [i_, vp_, vp_, vp_, vp_, d_, d_, i_, d_, d_, d_, i_, i_, vp_]
    return hs


@pytest.mark.parametrize('waveno', [0, 1])
def test_host_replay_of_the_per_row_form_equals_the_uniform_form(sets_sim, waveno):
    """Three models of different depth in one block, each at the ray parameter of its own set (the table holds a fourth
    that nobody uses, and the models' sets are not in table order): phases 1-3 of the per-row form give, for every
    model, the spectrum of the uniform form run on that model alone at that p -- bit for bit.  Pins the scalar slot
    that carries p^2 from phase 2 to phase 3, the model-to-set mapping and the late fetch of the filter factor."""
    from bayhunter_amd.synthetic import draw_models
    M, L, nsamp = 3, 12, 512
    H, VP, VS, RHO, nl = draw_models(M, (4, L), seed=31, Lmax=L)
    H, VP, VS, RHO = (np.ascontiguousarray(a, dtype=np.float64) for a in (H, VP, VS, RHO))
    nl = np.ascontiguousarray(nl, dtype=np.int32)
    assert len(set(nl)) > 1 and nl.max() <= L
    table = np.array([8.7, 4.3, 9.9, 6.1])
    set_id = np.array([3, 0, 1], dtype=np.int32)
    nfreq = nsamp // 2 + 1
    spec, bad = np.full((M, nfreq, 2), 7.0), np.full(M, -1, dtype=np.int32)
    args = (1.0, nsamp, 5.0, 5.0, -1.0, waveno, 201)
    nact = sets_sim.hs_rf_sets_spectra(M, L, nl.ctypes.data, H.ctypes.data, VP.ctypes.data, VS.ctypes.data, RHO.ctypes.data,
                                       4, table.ctypes.data, set_id.ctypes.data, *args, spec.ctypes.data, bad.ctypes.data)
    assert 0 < nact <= nfreq and not bad.any()
    for m in range(M):
        want = np.full((nfreq, 2), 7.0)
        n = int(nl[m])
        one = [np.ascontiguousarray(a[m, :n]) for a in (H, VP, VS, RHO)]
        assert sets_sim.hs_rf_spectrum(n, *[a.ctypes.data for a in one], float(table[set_id[m]]), *args,
                                       want.ctypes.data) == nact
        assert np.isfinite(want).all()
        assert spec[m].tobytes() == want.tobytes(), m
    assert not np.array_equal(spec[0, :nact], spec[1, :nact])
    # one set and no index: every model takes table[0]; an index out of range: flagged, NaN, the table not read
    one_p = np.array([6.4])
    sets_sim.hs_rf_sets_spectra(M, L, nl.ctypes.data, H.ctypes.data, VP.ctypes.data, VS.ctypes.data, RHO.ctypes.data,
                                1, one_p.ctypes.data, None, *args, spec.ctypes.data, bad.ctypes.data)
    want = np.zeros((nfreq, 2))
    sets_sim.hs_rf_spectrum(int(nl[2]), *[np.ascontiguousarray(a[2, :nl[2]]).ctypes.data for a in (H, VP, VS, RHO)], 6.4,
                            *args, want.ctypes.data)
    assert spec[2].tobytes() == want.tobytes()
    wrong = np.array([0, 4, -1], dtype=np.int32)
    sets_sim.hs_rf_sets_spectra(M, L, nl.ctypes.data, H.ctypes.data, VP.ctypes.data, VS.ctypes.data, RHO.ctypes.data,
                                4, table.ctypes.data, wrong.ctypes.data, *args, spec.ctypes.data, bad.ctypes.data)
    assert list(bad) == [0, 1, 1]
    assert np.isfinite(spec[0]).all() and np.isnan(spec[1, :nact]).all() and np.isnan(spec[2, :nact]).all()


# ---- the C ABI, before any device call -----------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared(lib):
    from bayhunter_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read()
    for name in ('bh_rf_batch_sets', 'bh_eval_set_rf_slowness'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert ('int %s(' % name) in header.replace('int  ', 'int ')


def test_rf_batch_sets_validates_arguments_without_gpu(lib):
    from bayhunter_amd import _lib
    par = _lib.RfParams(6.4, 1.0, 5.0, 5.0, -1.0, 512, 0, 201, 0)

    def call(B=4, Lmax=10, stride=40, nsets=3, set_p=1, set_id=1, par=par, out_stride=201, nlay=1):
        return lib.bh_rf_batch_sets(B, Lmax, stride, nlay, 1, 1, 1, 1, None, None, par, nsets, set_p, set_id, 1,
                                    out_stride, None, 0, None)
    assert call(B=0) == _lib.BH_OK                                                   # nothing to do
    assert call(nsets=0) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert call(nsets=-1, B=0) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert call(set_p=None) == _lib.BH_ERR_ARG and b'set_p' in lib.bh_last_error()
    assert call(set_id=None) == _lib.BH_ERR_ARG and b'set_id' in lib.bh_last_error()
    assert call(par=None) == _lib.BH_ERR_ARG and b'par' in lib.bh_last_error()
    assert call(nlay=None) == _lib.BH_ERR_ARG and b'NULL' in lib.bh_last_error()
    assert call(stride=9) == _lib.BH_ERR_ARG and b'model_stride' in lib.bh_last_error()
    assert call(out_stride=200) == _lib.BH_ERR_ARG and b'output row' in lib.bh_last_error()
    for field, value, word in (('nsamp', 500, b'nsamp'), ('waveno', 2, b'waveno'), ('gauss', 0.0, b'gauss')):
        bad = _lib.RfParams(6.4, 1.0, 5.0, 5.0, -1.0, 512, 0, 201, 0)
        setattr(bad, field, value)
        assert call(par=bad) == _lib.BH_ERR_ARG and word in lib.bh_last_error()


def test_eval_set_rf_slowness_validates_arguments_without_gpu(lib):
    from bayhunter_amd import _lib
    p = np.full((3, 1), 6.4)
    assert lib.bh_eval_set_rf_slowness(None, 0, p.ctypes.data) == _lib.BH_ERR_ARG and b'nsets' in lib.bh_last_error()
    assert lib.bh_eval_set_rf_slowness(None, 3, None) == _lib.BH_ERR_ARG and b'NULL' in lib.bh_last_error()
    assert lib.bh_eval_set_rf_slowness(None, 3, p.ctypes.data) == _lib.BH_ERR_ARG and b'plan is NULL' in lib.bh_last_error()
