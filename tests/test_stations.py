"""Station pool (bayhunter_amd/stations.py), CPU tier: the chains of many stations in one lock-step pool, every
row evaluated against its own station's observed data (here by one CPU-oracle evaluator per station).

A model's forward row and likelihood do not depend on the batch it is in, so every comparison with the
single-station `ChainPool` is exact: there is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import reference_chain as rc  # noqa: E402
from chain_scenario import CASES, oracle_evaluator  # noqa: E402
from station_scenario import make_stations, station_evaluator  # noqa: E402

DATA = os.path.join(GOLDEN, 'tutorial_observed')
KEYS = ('models', 'likes', 'misfits', 'noise', 'vpvs', 'iter')
needs_ref = pytest.mark.skipif(not rc.available(), reason='reference tree not present')


def _case(name, burnin, main):
    case = CASES[name]
    ip = dict(case['initparams'], iter_burnin=burnin, iter_main=main)
    return ip, case['priors']


def _station_pool(oracle, name, S, c, random_seeds, burnin=90, main=50, yerr=True, **kw):
    from bayhunter_amd.stations import StationPool
    ip, priors = _case(name, burnin, main)
    stations = make_stations(DATA, S, oracle=oracle, yerr=yerr)
    ev = station_evaluator([oracle_evaluator(j) for j in stations])
    return StationPool(stations, ip, priors, chains_per_station=c, random_seeds=random_seeds, evaluator=ev,
                       nmodels=burnin + main + 1, **kw)


def _single_pools(oracle, name, S, c, random_seeds, burnin=90, main=50, yerr=True):
    from bayhunter_amd.chains import ChainPool
    ip, priors = _case(name, burnin, main)
    out = []
    for s, joint in enumerate(make_stations(DATA, S, oracle=oracle, yerr=yerr)):
        out.append(ChainPool(joint, ip, priors, random_seed=random_seeds[s], nchains=c, evaluator=oracle_evaluator(joint),
                             nmodels=burnin + main + 1).run())
    return out


def _assert_station_equals(view, single):
    for k in KEYS:
        assert np.array_equal(getattr(view, k), getattr(single, k), equal_nan=True), k
    for a, b in zip(view.counters(), single.counters()):
        assert np.array_equal(a, b)
    assert np.array_equal(view.seeds, single.seeds)


@pytest.fixture(scope='module')
def singles(oracle):
    return _single_pools(oracle, 'tutorial', 3, 3, [7, 8, 9])


@pytest.mark.parametrize('kw', [dict(), dict(lookahead=4), dict(groups=2), dict(groups=2, lookahead=3)],
                         ids=['plain', 'lookahead', 'groups', 'groups_lookahead'])
def test_station_chains_are_the_single_station_pools_chains(oracle, singles, kw):
    """3 stations x 3 chains of the tutorial set-up (dense Gaussian RF noise, yerr-scaled dispersion noise) in one
    pool = three ChainPools with the same random seeds, array for array; also with a look-ahead and with two chain
    groups, whose boundary (chain 4) falls inside station 1."""
    pool = _station_pool(oracle, 'tutorial', 3, 3, [7, 8, 9], **kw).run()
    assert pool.nchains == 9 and pool.pool.lookahead == kw.get('lookahead', 1)
    if 'groups' in kw:
        assert [(g.first, g.last) for g in pool.pool.groups] == [(0, 4), (4, 9)]
    for s in range(3):
        _assert_station_equals(pool.station(s), singles[s])
    # the stations' data differ, and so do their chains (with equal seeds too: see the next test)
    assert not np.array_equal(pool.station(0).likes, pool.station(1).likes, equal_nan=True)
    pool.close()
    _assert_station_equals(pool.station(2), singles[2])          # a closed pool keeps its results


def test_different_data_give_different_chains_and_seeds_are_per_station(oracle):
    """Two stations with the SAME random seed start from the same models and draw the same numbers: whatever
    differs between their chains comes from their observed data.  Station 0's chains do not depend on which
    stations share the pool."""
    a = _station_pool(oracle, 'fixednoise', 2, 3, [5, 5], yerr=False, burnin=60, main=30).run()
    s0, s1 = a.station(0), a.station(1)
    assert np.array_equal(s0.seeds, s1.seeds)
    assert np.array_equal(s0.models[:, 0], s1.models[:, 0], equal_nan=True)           # same initial models
    assert not np.array_equal(s0.likes[:, 0], s1.likes[:, 0])                         # other data: other likelihood
    assert not np.array_equal(s0.likes, s1.likes, equal_nan=True) and not np.array_equal(s0.misfits, s1.misfits, equal_nan=True)
    b = _station_pool(oracle, 'fixednoise', 3, 3, [5, 11, 12], yerr=False, burnin=60, main=30).run()
    _assert_station_equals(b.station(0), s0)
    # explicit per-chain seeds; names from a mapping
    from bayhunter_amd.stations import StationPool
    ip, priors = _case('fixednoise', 60, 30)
    stations = make_stations(DATA, 2, oracle=oracle)
    ev = station_evaluator([oracle_evaluator(j) for j in stations])
    c = StationPool(dict(AAA=stations[0], BBB=stations[1]), ip, priors, seeds=[s0.seeds, [1, 2, 3]], evaluator=ev,
                    nmodels=91).run()
    assert c.names == ['AAA', 'BBB'] and c.chains_per_station == 3
    _assert_station_equals(c.station('AAA'), s0)
    with pytest.raises(KeyError):
        c.station('CCC')
    with pytest.raises(IndexError):
        c.station(2)


def test_three_argument_evaluators_and_plain_pools_are_untouched(oracle):
    """A function of three arguments gets what it always got, from a ChainPool and from a StationPool."""
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool
    ip, priors = _case('fixednoise', 20, 10)
    seen = []

    def three(packed, nlay, noise):
        seen.append(3)
        return -np.abs(packed[:, 2, 0] - 3.0), np.ones((packed.shape[0], 3))

    def four(packed, nlay, noise, station):
        seen.append(station.copy())
        return -np.abs(packed[:, 2, 0] - 3.0 - 0.1 * station), np.ones((packed.shape[0], 3))
    stations = make_stations(DATA, 2)
    ChainPool(stations[0], ip, priors, seeds=[1, 2], evaluator=three, nmodels=31).run()
    assert seen and all(x == 3 for x in seen)
    del seen[:]
    StationPool(stations, ip, priors, seeds=[[1, 2], [3, 4]], evaluator=three, nmodels=31).run()
    assert seen and all(isinstance(x, int) for x in seen)
    del seen[:]
    pool = StationPool(stations, ip, priors, seeds=[[1, 2], [3, 4]], evaluator=four, nmodels=31, lookahead=3).run()
    assert seen and all(x.dtype == np.int32 and set(x) <= {0, 1} for x in seen)
    # with a look-ahead a chain has several rows per call, each with its own station
    assert max(x.size for x in seen) > 4 and any(np.count_nonzero(x == 1) > 2 for x in seen)
    assert pool.advance()[2] == sum(x.size for x in seen[1:])


def test_refusals_name_station_and_property(oracle):
    from bayhunter_amd.stations import StationPool
    ip, priors = _case('tutorial', 20, 10)

    def build(stations, **kw):
        return StationPool(stations, ip, priors, chains_per_station=2, random_seeds=list(range(len(stations))),
                           evaluator=lambda p, n, z, s: None, **kw)
    ok = make_stations(DATA, 3, yerr=True)
    build(ok).close()
    st = make_stations(DATA, 3, yerr=True)                       # other periods
    t = st[2].targets[0]
    t.obsdata.x = t.obsdata.x * 1.01
    with pytest.raises(ValueError, match=r"station 'st002'.*target 0.*x axis"):
        build(st)
    for key, val in (('p', 7.0), ('gauss', 2.0)):                # other slowness / Gauss factor of the receiver function
        st = make_stations(DATA, 2, yerr=True)
        st[1].targets[1].moddata.plugin.set_modelparams(**{key: val})
        with pytest.raises(ValueError, match=r"station 'st001'.*target 1.*%r" % key):
            build(st)
    st = make_stations(DATA, 2, yerr=True)
    st[1].targets[0].moddata.plugin.set_modelparams(mode=2)
    with pytest.raises(ValueError, match=r"station 'st001'.*target 0.*'mode'"):
        build(st)
    st = make_stations(DATA, 2, yerr=True)                       # other number of targets
    from bayhunter_amd import targets as T
    st[1] = T.JointTarget(st[1].targets[:1])
    with pytest.raises(ValueError, match=r"station 'st001'.*number of targets"):
        build(st)
    st = make_stations(DATA, 3, yerr=True)                       # yerr at one station, none at another
    st[1].targets[0].obsdata.yerr = np.full(st[1].targets[0].obsdata.x.size, np.nan)
    with pytest.raises(ValueError, match=r"station 'st001'.*target 0.*covariance model"):
        build(st)
    st = make_stations(DATA, 2, yerr=True)
    with pytest.raises(ValueError, match='st001'):
        build(dict(named=st[0], st001=T.JointTarget(st[1].targets[::-1])))
    with pytest.raises(ValueError, match='shard'):
        build(ok, shard=(0, 2))
    with pytest.raises(ValueError, match='one per station'):
        StationPool(ok, ip, priors, chains_per_station=2, random_seeds=[1, 2], evaluator=lambda p, n, z, s: None)
    with pytest.raises(ValueError, match='nstations'):
        StationPool(ok, ip, priors, seeds=[[1, 2]], evaluator=lambda p, n, z, s: None)


def test_save_writes_one_single_station_directory_per_station(oracle, singles, tmp_path):
    """save(): <savepath>/<station>/data/c%03d_... numbered from 0 and <station>_config.pkl with the station's own
    targets -- the .npy files are byte for byte the files of the single-station pools; outliers() of a view are
    the single pool's."""
    import pickle
    pool = _station_pool(oracle, 'tutorial', 3, 3, [7, 8, 9]).run()
    n = pool.save(str(tmp_path / 'all'))
    total = 0
    for s, name in enumerate(pool.names):
        total += singles[s].save(str(tmp_path / 'one' / name))
        mine, ref = tmp_path / 'all' / name / 'data', tmp_path / 'one' / name / 'data'
        files = sorted(f for f in os.listdir(str(ref)) if f.endswith('.npy'))
        assert files and files == sorted(f for f in os.listdir(str(mine)) if f.endswith('.npy'))
        assert files[0].startswith('c000_')
        for f in files:
            assert (mine / f).read_bytes() == (ref / f).read_bytes(), (name, f)
        with open(str(mine / ('%s_config.pkl' % name)), 'rb') as fh:
            cfg = pickle.load(fh)
        assert cfg['targetrefs'] == ['rdispph', 'prf'] and cfg['initparams']['station'] == name
        assert np.array_equal(cfg['targets'][0].obsdata.y, pool.stations[s].targets[0].obsdata.y)
        assert np.array_equal(pool.station(s).outliers(), singles[s].outliers())
        for i in range(3):
            assert np.array_equal(pool.station(s).final(i), singles[s].final(i), equal_nan=True)
    assert n == total
    # saving leaves the covariance models selected (save() resets and restores them, like ChainPool.save)
    assert [t.covmodel for t in pool.stations[1].targets] == [t.covmodel for t in singles[1].targets.targets]


@needs_ref
def test_reference_plotfromstorage_reads_a_station_directory(oracle, tmp_path):
    """The reference's own PlotFromStorage (unmodified) opens the directory of one station of a pool."""
    pool = _station_pool(oracle, 'fixednoise', 2, 4, [5, 6], yerr=False, burnin=150, main=100).run()
    pool.save(str(tmp_path))
    data = str(tmp_path / 'st001' / 'data')
    PlotFromStorage = rc.load_plot_from_storage()
    obj = PlotFromStorage(os.path.join(data, 'st001_config.pkl'))
    assert obj.ntargets == 2 and obj.refs == ['rdispph', 'prf', 'joint']
    assert len(obj.likefiles[1]) == 4 and len(obj.modfiles[0]) == 4
    chains, nmodels = obj._get_chaininfo()
    view = pool.station('st001')
    assert chains == [0, 1, 2, 3] and nmodels == [view.weighted(i)[2][1].size for i in range(4)]
    obj.save_final_distribution(maxmodels=200, dev=0.5)
    likes = np.load(os.path.join(data, 'c_likes.npy'))
    stored = np.concatenate([view.weighted(i)[2][1] for i in range(4)])
    assert likes.size and np.all(np.isin(likes, stored))
