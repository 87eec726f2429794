"""GPU tier of the scalar-parameter posterior (bh_hist2d_sets, bayhunter_amd/scalars.py, ChainPool.scalars,
StationPool.scalars, StationPool.moho(tradeoff=True)) against the numpy restatement (tests/scalars_ref.py).

Counts, order statistics, edges, modes and medians are compared bit for bit; mean and standard deviation within
tests/datafits_tolerances.py (only the order of a sum differs)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import scalars_ref as ref  # noqa: E402
from datafits_tolerances import STD_ATOL, STD_RTOL, check_mean  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 505)                 # 700 rows in 7 sets
PAIRS = [(0, 1), (1, 0), (2, 2), (3, 4)]


def hist2d(D, w, start, pairs, edges, pad=0, expect=0):
    """bh_hist2d_sets over the host matrix D (uploaded, `pad` unused columns beyond it) -> hist, or the error text."""
    import torch
    from bayhunter_amd import _lib
    lib = _lib.load()
    R, K = D.shape
    t = torch.full((R, K + pad), 7.0, dtype=torch.float64, device='cuda')
    t[:, :K] = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float64)).cuda()
    dw = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.int32)).cuda()
    start = np.ascontiguousarray(start, dtype=np.int64)
    pr = np.ascontiguousarray(pairs, dtype=np.int32)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    nb = edges.shape[2] - 1
    hist = np.full((start.size - 1, len(pairs), nb, nb), -1, dtype=np.int64)
    rc = lib.bh_hist2d_sets(t.data_ptr(), R, K + pad, K, None if dw is None else dw.data_ptr(), start.ctypes.data,
                            start.size - 1, pr.ctypes.data, len(pairs), edges.ctypes.data, nb + 1, hist.ctypes.data,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == expect, lib.bh_last_error()
    return hist if rc == 0 else lib.bh_last_error().decode()


def set_edges(D, w, start, nb):
    """Per set and column np.histogram's edges over the set's finite values of positive weight."""
    S, K = len(start) - 1, D.shape[1]
    w = np.ones(D.shape[0], dtype=np.int64) if w is None else np.asarray(w)
    edges = np.zeros((S, K, nb + 1))
    edges[:] = np.arange(nb + 1)
    for s in range(S):
        for c in range(K):
            v = D[start[s]:start[s + 1], c][w[start[s]:start[s + 1]] > 0]
            v = v[~np.isnan(v)]
            if v.size:
                edges[s, c] = np.histogram(v, bins=nb)[1]
    return edges


@pytest.fixture(scope='module')
def rows_case():
    rs = np.random.RandomState(31)
    start = np.concatenate(([0], np.cumsum(SIZES)))
    D = rs.randn(700, 5) * np.array([1., 3., .1, 10., 1.]) + np.arange(5)
    D[:, 4] = np.round(D[:, 4])                    # few distinct values: many of them on edges
    for c in range(5):
        D[rs.rand(700) < 0.05, c] = np.nan         # per column independently
    w = rs.randint(0, 6, 700).astype(np.int32)
    assert (w == 0).sum() > 50
    return D, w, start


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('nb', [1, 3, 20, 50, 64])
def test_hist2d_sets_equals_the_restatement(lib, rows_case, nb, weighted):
    D, w, start = rows_case
    w = w if weighted else None
    edges = set_edges(D, w, start, nb)
    edges[6, 3] = np.linspace(0., 12., nb + 1)     # edges that leave values outside on both sides
    want = ref.hist2d_sets(D, w, start, PAIRS, edges)
    assert want[0].sum() == 0 and want[6].sum() > 1000 and want[6, 3].sum() < want[6, 0].sum()
    got = hist2d(D, w, start, PAIRS, edges, pad=3)
    assert np.array_equal(got, want)
    assert np.array_equal(hist2d(D, w, start, PAIRS, edges), got)             # two runs, and no stride in the result


def test_sixteen_pairs_at_64_bins_come_in_groups(lib, rows_case):
    D, w, start = rows_case
    edges = set_edges(D, w, start, 64)
    pairs = PAIRS + [(a, b) for a in range(5) for b in range(5) if (a, b) not in PAIRS][:12]
    assert len(pairs) == 16 and len(set(pairs)) == 16
    got = hist2d(D, w, start, pairs, edges)
    assert np.array_equal(got[:, :4], hist2d(D, w, start, PAIRS, edges))
    assert np.array_equal(got, ref.hist2d_sets(D, w, start, pairs, edges))


def test_a_long_set_is_split_over_blocks(lib):
    rs = np.random.RandomState(32)
    R = 40000
    D = rs.randn(R, 3) + np.array([0., 5., -5.])
    D[rs.rand(R) < 0.01, 1] = np.nan
    w = rs.randint(0, 4, R).astype(np.int32)
    for start in ([0, R], [0, 17, R - 4097, R]):
        edges = set_edges(D, w, start, 20)
        pairs = [(0, 1), (2, 0), (1, 1)]
        want = ref.hist2d_sets(D, w, start, pairs, edges)
        got = hist2d(D, w, start, pairs, edges)
        assert np.array_equal(got, want) and np.array_equal(hist2d(D, w, start, pairs, edges), got)


def test_sums_are_64_bit(lib):
    D = np.tile([[1.5, 3.]], (8, 1))
    edges = np.tile(np.array([0., 1., 2., 4.]), (1, 2, 1))
    got = hist2d(D, np.full(8, 1 << 30, dtype=np.int32), [0, 8], [(0, 1)], edges)
    assert got[0, 0, 1, 2] == 1 << 33 and got.sum() == 1 << 33


def test_a_negative_weight_is_refused(lib, rows_case):
    from bayhunter_amd import _lib
    D, w, start = rows_case
    w = w.copy()
    w[start[6] + 17] = -1
    msg = hist2d(D, w, start, PAIRS, set_edges(D, None, start, 20), expect=_lib.BH_ERR_ARG)
    assert 'negative weight' in msg


# ---- the statistic ------------------------------------------------------------------------------------------

TAGS = ['f4', 'f4', 'f8', 'f8', 'f8', 'n', 'f4', 'pair']
NAMES = ['a4', 'b4', 'c8', 'd8', 'e8', 'count', 'const', 'depth']
COLPAIRS = [('depth', 'b4'), ('c8', 'd8'), ('count', 'a4'), ('const', 'e8'), ('depth', 'depth')]


def mixed_columns(rs, R):
    """Two float32 columns, three float64, a count, a constant float32 column; a pairs-only column with NaN."""
    data = np.zeros((R, 8))
    data[:, 0] = (rs.randn(R) * 30 - 200).astype(np.float32)
    data[:, 1] = np.round(rs.rand(R) * 0.4 + 1.5, 2).astype(np.float32)       # many ties
    data[:, 2:5] = rs.randn(R, 3) * np.array([1e-3, 1., 50.]) + np.array([0.01, 0., 7.])
    data[:, 5] = rs.randint(2, 9, R)
    data[:, 6] = np.float32(0.35)
    data[:, 7] = np.where(rs.rand(R) < 0.3, np.nan, rs.rand(R) * 30 + 20)
    return data


def check_against_the_restatement(got, data, w, nbins, pair_bins):
    want = ref.summarize(data, TAGS, NAMES, w, nbins, COLPAIRS, pair_bins)

    def mean_std(g, wnt, name):
        print(name, g['mean'], wnt['mean'], g['std'], wnt['std'])
        np.testing.assert_allclose(g['std'], wnt['std'], rtol=STD_RTOL, atol=STD_ATOL)
    ref.assert_record(got, want, NAMES, 7, mean_std)
    ww = np.ones(data.shape[0], dtype=np.int64) if w is None else np.asarray(w)
    check_mean(np.array([got[n]['mean'] for n in NAMES[:7]]), data[:, :7], ww)
    assert want['const']['constant'] and want['const']['hist'][1].size == 4
    assert want['a4']['constant'] == (np.unique(data[ww > 0, 0]).size == 1)        # (the set of one row)
    assert want['a4']['hist'][1].dtype == np.float32 and want['c8']['hist'][1].dtype == np.float64


@pytest.mark.parametrize('odd', [False, True])
def test_summarize_equals_the_restatement(lib, odd):
    from bayhunter_amd import scalars
    rs = np.random.RandomState(33)
    R = 701
    data = mixed_columns(rs, R)
    w = rs.randint(0, 5, R).astype(np.int32)
    if (w.sum() % 2 == 1) != odd:
        w[np.argmax(w > 0)] += 1
    assert (w.sum() % 2 == 1) == odd
    cols = scalars.Columns(data, TAGS, NAMES)
    got = scalars.summarize(cols, w, nbins=20, pairs=COLPAIRS, pair_bins=50)
    check_against_the_restatement(got, data, w, 20, 50)
    assert got['nmodels_depth'] + got['nexcluded_depth'] == got['nmodels'] == w.sum()
    # without weights; a constant count; the pairs-only column without a value
    data[:, 5] = 4.
    check_against_the_restatement(scalars.summarize(cols, None, nbins=7, pairs=COLPAIRS, pair_bins=9), data, None, 7, 9)
    data[:, 7] = np.nan
    hole = scalars.summarize(cols, w, pairs=COLPAIRS, pair_bins=50)
    check_against_the_restatement(hole, data, w, 20, 50)
    assert hole['nmodels_depth'] == 0 and hole['pairs'][('depth', 'b4')]['counts'].sum() == 0
    assert np.isnan(hole['pairs'][('depth', 'b4')]['mode']).all() and hole['pairs'][('c8', 'd8')]['counts'].sum() == w.sum()


def test_summarize_sets_equals_summarize_on_every_set(lib):
    from bayhunter_amd import scalars
    rs = np.random.RandomState(34)
    sizes = (0, 1, 2, 150, 3, 544)                 # 700 rows; the set of two rows has no weight
    start = np.concatenate(([0], np.cumsum(sizes)))
    data = mixed_columns(rs, 700)
    w = rs.randint(0, 5, 700).astype(np.int32)
    w[start[1]] = 3
    w[start[2]:start[3]] = 0
    w[start[4]:start[5]] = [1, 0, 1]
    data[start[4]:start[5], 7] = np.nan            # a set without a value in the pairs-only column
    totals = [int(w[a:b].sum()) for a, b in zip(start[:-1], start[1:])]
    assert {t % 2 for t in totals if t} == {0, 1}, totals
    res = scalars.summarize_sets(scalars.Columns(data, TAGS, NAMES), start, w, nbins=20, pairs=COLPAIRS, pair_bins=50)
    assert sorted(res.failed) == [0, 2] and all('empty selection' in m for m in res.failed.values())
    for z in range(len(sizes)):
        sl = slice(start[z], start[z + 1])
        if z in res.failed:
            assert res[z] is None and ref.summarize(data[sl], TAGS, NAMES, w[sl]) is None
            continue
        check_against_the_restatement(res[z], data[sl], w[sl], 20, 50)
        one = scalars.summarize(scalars.Columns(data[sl], TAGS, NAMES), w[sl], nbins=20, pairs=COLPAIRS, pair_bins=50)
        assert_same_record(res[z], one)
    with pytest.raises(ValueError, match='empty selection'):
        scalars.summarize(scalars.Columns(data[start[2]:start[3]], TAGS, NAMES), w[start[2]:start[3]])


def assert_same_record(a, b):
    """Two summarize() dicts, every field bit for bit (mean and std too)."""
    assert list(a) == list(b)
    for k in a:
        if k == 'pairs':
            assert list(a[k]) == list(b[k])
            for p in a[k]:
                assert np.array_equal(a[k][p]['counts'], b[k][p]['counts']), p
                for f in ('xedges', 'yedges', 'mode'):
                    assert ref.same(a[k][p][f], b[k][p][f]), (p, f)
        elif isinstance(a[k], dict):
            for f in ('median', 'mean', 'std', 'min', 'max', 'mode', 'constant'):
                assert ref.same(a[k][f], b[k][f]), (k, f, a[k][f], b[k][f])
            assert np.array_equal(a[k]['hist'][0], b[k]['hist'][0]), k
            assert a[k]['hist'][1].dtype == b[k]['hist'][1].dtype and ref.same(a[k]['hist'][1], b[k]['hist'][1]), k
        else:
            assert np.array_equal(a[k], b[k]), k


# ---- pools --------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def station_pool(lib):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=150, iter_main=100)
    stations = make_stations(os.path.join(GOLDEN, 'tutorial_observed'), 3, refs=case.get('refs', ('rdispph', 'prf')), yerr=True)
    with StationPool(dict(zip(['AAA', 'BBB', 'CCC'], stations)), ip, case['priors'], chains_per_station=4,
                     random_seeds=[21, 22, 23], nmodels=251) as pool:
        pool.run()
    pool.pool.initparams['maxmodels'] = 13                  # thinning > 1 in save()
    return pool


POOL_MOHOVS = 3.6            # low enough that short chains from the prior have models with a Moho


def test_station_pool_scalars_equal_every_station_views(station_pool):
    pool = station_pool
    refs = [t.ref for t in pool.stations[0].targets]
    pairs = [('moho', 'vpvs'), ('sigma:%s' % refs[1], 'sigma:%s' % refs[0]), ('nlayers', 'like')]
    z = pool.pool.priors['z']
    for kw in (dict(selection='weighted'), dict(selection='saved', exclude_outliers=False)):
        kw = dict(kw, dev=0.5, pairs=pairs, pair_bins=30, moho=z, mohovs=POOL_MOHOVS)
        res = pool.scalars(**kw)
        assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and sorted(res.stations) == res.names
        assert res.columns == ['like', 'misfit:%s' % refs[0], 'misfit:%s' % refs[1], 'misfit:joint', 'vpvs',
                               'corr:%s' % refs[0], 'sigma:%s' % refs[0], 'corr:%s' % refs[1], 'sigma:%s' % refs[1], 'nlayers']
        assert (res.nmodels_moho > 0).any() and list(res.pairs) == pairs
        for s, name in enumerate(res.names):
            one = pool.station(name).scalars(**kw)
            assert_same_record(res.stations[name], one)
            assert res.nmodels[s] == one['nmodels'] and res.nmodels_moho[s] == one['nmodels_moho']
            assert res.nexcluded_moho[s] == one['nexcluded_moho'] == one['nmodels'] - one['nmodels_moho']
            for c in res.columns:
                for f in ('median', 'mean', 'std', 'min', 'max', 'mode'):
                    assert ref.same(res.stats[c][f][s], one[c][f]), (name, c, f)
                nb = one[c]['hist'][0].size
                assert np.array_equal(res.stats[c]['hist'][s, :nb], one[c]['hist'][0])
                assert ref.same(res.stats[c]['edges'][s, :nb + 1], one[c]['hist'][1])
                assert one[c]['hist'][0].sum() == one['nmodels']
            assert res.stats['vpvs']['hist'].shape == (3, 20) and res.stats['vpvs']['edges'].shape == (3, 21)
            for p in pairs:
                assert np.array_equal(res.pairs[p]['counts'][s], one['pairs'][p]['counts'])
                assert ref.same(res.pairs[p]['mode'][s], one['pairs'][p]['mode'])
                assert ref.same(res.pairs[p]['xedges'][s], one['pairs'][p]['xedges'])
            assert one['pairs'][pairs[0]]['counts'].sum() == one['nmodels_moho']
            assert one['pairs'][pairs[2]]['counts'].sum() == one['nmodels']
        # runs of whole stations: no result depends on them
        split = pool.scalars(max_rows=1, **kw)
        for name in res.names:
            assert_same_record(split.stations[name], res.stations[name])


def test_chain_pool_scalars_by_chain_equal_the_restatement_on_the_saved_files(station_pool, tmp_path):
    from bayhunter_amd import scalars
    view = station_pool.station('BBB')
    view.save(str(tmp_path))
    refs = [t.ref for t in view.targets.targets]
    names, tags = scalars.NAMES(2, refs), scalars.TAGS(2)
    pairs = [('nlayers', 'like'), ('sigma:%s' % refs[1], 'sigma:%s' % refs[0])]
    got = view.scalars(selection='saved', exclude_outliers=False, by_chain=True, pairs=pairs, pair_bins=25)
    assert len(got) == 4 and not got.failed and np.array_equal(got.chains, np.arange(4))
    for i in range(4):
        load = lambda what: np.load(str(tmp_path / 'data' / ('c%.3d_p2%s.npy' % (i, what))))
        likes, misfits, vpvs, noise, models = (load(k) for k in ('likes', 'misfits', 'vpvs', 'noise', 'models'))
        assert likes.dtype == vpvs.dtype == np.float32 and misfits.dtype == noise.dtype == models.dtype == np.float64
        layers = np.array([(m[~np.isnan(m)].size / 2 - 1) for m in models])          # Plotting.py:612-613
        data = np.column_stack((likes, misfits, vpvs, noise, layers))
        want = ref.summarize(data, tags, names, None, 20, pairs, 25)
        ref.assert_record(got[i], want, names, len(names), lambda g, w, name: (
            np.testing.assert_allclose(g['mean'], w['mean'], rtol=1e-12, atol=0),
            np.testing.assert_allclose(g['std'], w['std'], rtol=STD_RTOL, atol=STD_ATOL)))
        assert got[i]['nmodels'] == likes.size <= 13
    # one set over all chains: the merged posterior of the same files
    allc = view.scalars(selection='saved', exclude_outliers=False, pairs=pairs, pair_bins=25)
    assert allc['nmodels'] == sum(g['nmodels'] for g in got) and np.array_equal(allc['chains'], np.arange(4))


def test_station_pool_moho_tradeoff_equals_every_station_views(station_pool):
    pool = station_pool
    plain = pool.moho(mohovs=POOL_MOHOVS, dev=0.5)
    assert sorted(vars(plain)) == sorted(['names', 'failed', 'nmodels', 'nexcluded', 'fraction', 'hist', 'edges', 'moho',
                                          'vs_crust', 'vs_last', 'vs_jump'])
    res = pool.moho(mohovs=POOL_MOHOVS, dev=0.5, tradeoff=True)
    assert sorted(set(vars(res)) - set(vars(plain))) == ['tradeoff'] and list(res.tradeoff) == ['vs_last', 'vs_crust', 'vs_jump']
    for k in ('nmodels', 'nexcluded', 'hist', 'edges'):
        assert np.array_equal(getattr(res, k), getattr(plain, k))
    for q in ('moho', 'vs_crust', 'vs_last', 'vs_jump'):
        for k in ('median', 'mean', 'std', 'min', 'max'):
            assert ref.same(getattr(res, q)[k], getattr(plain, q)[k])
    assert (res.nmodels > 0).any()
    for s, name in enumerate(res.names):
        for x, t in res.tradeoff.items():
            assert t['counts'].shape == (3, 50, 50) and t['xedges'].shape == t['yedges'].shape == (3, 51)
            if res.nmodels[s] == 0:
                assert t['counts'][s].sum() == 0 and np.isnan(t['xedges'][s]).all() and np.isnan(t['mode'][s]).all()
                continue
            one = pool.station(name).moho(mohovs=POOL_MOHOVS, dev=0.5)['tradeoff'][x]
            assert np.array_equal(t['counts'][s], one['counts']) and t['counts'][s].sum() == res.nmodels[s]
            assert ref.same(t['xedges'][s], one['xedges']) and ref.same(t['yedges'][s], one['yedges'])
            assert ref.same(t['mode'][s], one['mode'])
