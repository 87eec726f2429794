"""GPU tier of the Moho / crustal-velocity posterior (bh_moho_*, bayhunter_amd/moho.py, ChainPool.moho,
StationPool.moho) against the numpy restatement of the reference (tests/moho_ref.py).

Per-row values, counts, order statistics, edges and modes are compared bit for bit; mean and standard deviation
within tests/posterior_tolerances.py (only the order of a sum differs)."""
import glob
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import moho_ref as ref  # noqa: E402
from posterior_tolerances import MEAN_RTOL, STD_ATOL, STD_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu
WINDOW, MOHOVS, WIDTH = (20., 50.), 4.1, 40
STATS = ('median', 'mean', 'std', 'min', 'max')

_rows = {}


def case_rows(dtype):
    """The CPU tier's built cases and 4 099 random rows, with the restatement's D (computed once)."""
    key = np.dtype(dtype).name
    if key not in _rows:
        rs = np.random.RandomState(21 if key == 'float32' else 22)
        rows = np.concatenate((ref.built_cases(dtype, WIDTH, WINDOW, MOHOVS)[0], ref.random_rows(rs, 4099, WIDTH, dtype)))
        _rows[key] = (rows, ref.derive(rows, WINDOW, MOHOVS))
    return _rows[key]


def on_device(rows, pad=0):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    if pad:
        wide = torch.full((rows.shape[0], rows.shape[1] + pad), 7.0, dtype=t.dtype, device=t.device)
        wide[:, :rows.shape[1]] = t
        t = wide[:, :rows.shape[1]]
    return t


def device_D(rows, pad=0):
    import torch
    from bayhunter_amd import moho
    t = on_device(rows, pad)
    assert t.stride(0) == rows.shape[1] + pad
    D = moho.derive(t, WINDOW[0], WINDOW[1], MOHOVS, torch.cuda.current_stream().cuda_stream)
    return D.cpu().numpy()


def assert_bits(got, want):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)])


@pytest.mark.parametrize('pad', [0, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_rows_equal_the_restatement(lib, dtype, pad):
    rows, want = case_rows(dtype)
    has = ~np.isnan(want[:, 0])
    assert rows.shape[0] % 64 and 0.2 < has.mean() < 0.8
    assert_bits(device_D(rows, pad), want)
    for k in (1, 63, 257):
        assert_bits(device_D(rows[-k:], pad), want[-k:])


def assert_summary(got, want):
    assert got['nmodels'] == want['nmodels'] and got['nexcluded'] == want['nexcluded']
    for name in ref.NAMES:
        g, w = got[name], want[name]
        print(name, {k: (g[k], w[k]) for k in STATS})
        for k in ('median', 'min', 'max'):
            assert g[k] == w[k], (name, k)
        assert np.array_equal(g['hist'][0], w['hist'][0]) and np.array_equal(g['hist'][1], w['hist'][1]), name
        assert g['hist'][0].sum() == want['nmodels']
        np.testing.assert_allclose(g['mean'], w['mean'], rtol=MEAN_RTOL, atol=0)
        np.testing.assert_allclose(g['std'], w['std'], rtol=STD_RTOL, atol=STD_ATOL)
    assert list(got['tradeoff']) == list(ref.TRADEOFF)
    for name in ref.TRADEOFF:
        g, w = got['tradeoff'][name], want['tradeoff'][name]
        assert g['counts'].shape == w['counts'].shape and np.array_equal(g['counts'], w['counts']), name
        assert np.array_equal(g['xedges'], w['xedges']) and np.array_equal(g['yedges'], w['yedges']), name
        assert g['mode'] == w['mode'] and g['counts'].sum() == want['nmodels'], name


def weights_for(rs, R):
    w = rs.randint(0, 7, R).astype(np.int32)
    w[rs.rand(R) < 0.1] = 0
    return w


@pytest.mark.parametrize('dtype,R,nbins', [(np.float32, 4000, 50), (np.float64, 300, 50), (np.float32, 1500, 53)])
def test_summarize_equals_the_restatement_on_the_expansion(lib, dtype, R, nbins):
    from bayhunter_amd import moho
    assert (3 * 50 * 50 * 8 <= 64 * 1024) and (3 * 53 * 53 * 8 > 64 * 1024)       # 53 bins: the global-atomics form
    rows, D = case_rows(dtype)
    rows, D = rows[-R:], D[-R:]
    w = weights_for(np.random.RandomState(R), R)
    want = ref.statistics(D, w, nbins)
    assert want['nexcluded'] > 0 and (w == 0).any()
    got = moho.summarize(rows, w, WINDOW, MOHOVS, nbins=nbins)
    assert_summary(got, want)
    if nbins == 50 and dtype == np.float32:                 # no weights: every row once
        assert_summary(moho.summarize(rows, None, WINDOW, MOHOVS), ref.statistics(D, None, 50))


def test_summarize_with_one_moho_depth_and_with_none(lib):
    from bayhunter_amd import moho
    rs = np.random.RandomState(5)
    vs = np.stack((rs.uniform(2.5, 3.5, 200), rs.uniform(3.5, 4.0, 200), rs.uniform(4.2, 4.8, 200)), axis=1)
    rows = np.stack([ref.layered_row(v, [12., 33.], WIDTH, np.float32) for v in vs])
    w = weights_for(rs, 200)
    want = ref.summarize(rows, w, WINDOW, MOHOVS)
    assert want['moho']['min'] == want['moho']['max']                              # edges at +-0.5
    assert want['moho']['hist'][1][0] == want['moho']['min'] - 0.5
    assert_summary(moho.summarize(rows, w, WINDOW, MOHOVS), want)
    shallow = rows.copy()
    shallow[:, 2] = 3.9                                                             # nothing exceeds mohovs
    with pytest.raises(ValueError, match='mohovs = 4.1'):
        moho.summarize(shallow, w, WINDOW, MOHOVS)
    with pytest.raises(ValueError):
        ref.summarize(shallow, w, WINDOW, MOHOVS)


SIZES = (0, 1, 2, 64, 65, 300, 1000)


@pytest.fixture(scope='module')
def sets_case():
    rows, D = case_rows(np.float32)
    has = np.nonzero(~np.isnan(D[:, 0]))[0]
    start = np.concatenate(([0], np.cumsum(SIZES)))
    R = int(start[-1])
    rs = np.random.RandomState(6)
    pick = rs.randint(0, rows.shape[0], R)
    pick[start[1]] = has[0]                                  # the set of one row has a Moho
    pick[start[2]:start[3]] = has[1:3]
    none = np.nonzero(np.isnan(D[:, 0]))[0]
    pick[start[3]:start[4]] = none[rs.randint(0, none.size, 64)]                    # the set of 64 rows has none
    w = rs.randint(0, 7, R).astype(np.int32)
    w[start[1]:start[3]] = (3, 1, 2)
    return rows[pick], D[pick], w, start


def test_sets_equal_summarize_of_each_set(lib, sets_case):
    from bayhunter_amd import moho
    rows, D, w, start = sets_case
    S = len(SIZES)
    got = moho.summarize_sets(rows, start, w, WINDOW, MOHOVS, nbins=50)
    assert np.array_equal(got['edges'], np.linspace(WINDOW[0], WINDOW[1], 51)) and got['hist'].shape == (S, 50)
    holes = []
    for z in range(S):
        sl = slice(start[z], start[z + 1])
        E = np.repeat(D[sl], w[sl], axis=0)
        with_moho = int((~np.isnan(E[:, 0])).sum())
        assert got['nmodels'][z] == with_moho and got['nexcluded'][z] == E.shape[0] - with_moho
        assert np.array_equal(got['hist'][z], np.histogram(E[~np.isnan(E[:, 0]), 0], bins=got['edges'])[0])
        if with_moho == 0:
            holes.append(z)
            assert all(np.isnan(got[name][k][z]) for name in ref.NAMES for k in STATS) and not got['hist'][z].any()
            assert np.isnan(got['fraction'][z]) if E.shape[0] == 0 else got['fraction'][z] == 0.
            if E.shape[0]:
                with pytest.raises(ValueError):
                    moho.summarize(rows[sl], w[sl], WINDOW, MOHOVS)
            continue
        one = moho.summarize(rows[sl], w[sl], WINDOW, MOHOVS)
        assert got['nmodels'][z] == one['nmodels'] and got['nexcluded'][z] == one['nexcluded']
        assert got['fraction'][z] == one['nmodels'] / float(one['nmodels'] + one['nexcluded'])
        for name in ref.NAMES:
            for k in ('median', 'min', 'max'):
                assert got[name][k][z] == one[name][k], (z, name, k)
            print(z, name, got[name]['mean'][z], one[name]['mean'], got[name]['std'][z], one[name]['std'])
            np.testing.assert_allclose(got[name]['mean'][z], one[name]['mean'], rtol=MEAN_RTOL, atol=0)
            np.testing.assert_allclose(got[name]['std'][z], one[name]['std'], rtol=STD_RTOL, atol=STD_ATOL)
    assert holes == [0, 3]
    # a set's numbers do not depend on its neighbours
    for z in range(1, S):
        sl = slice(start[z], start[z + 1])
        alone = moho.summarize_sets(rows[sl], [0, SIZES[z]], w[sl], WINDOW, MOHOVS, nbins=50)
        assert alone['nmodels'][0] == got['nmodels'][z] and np.array_equal(alone['hist'][0], got['hist'][z])
        for name in ref.NAMES:
            for k in STATS:
                assert np.array_equal(alone[name][k][0], got[name][k][z], equal_nan=True), (z, name, k)
    again = moho.summarize_sets(rows, start, w, WINDOW, MOHOVS, nbins=50)
    assert np.array_equal(again['hist'], got['hist'])
    for name in ref.NAMES:
        for k in STATS:
            assert np.array_equal(again[name][k], got[name][k], equal_nan=True)
    # more bins than the kernel keeps in LDS (2 048): the histogram through global atomics, nothing else moves
    fine = moho.summarize_sets(rows, start, w, WINDOW, MOHOVS, nbins=2100)
    for z in range(S):
        sl = slice(start[z], start[z + 1])
        E = np.repeat(D[sl], w[sl], axis=0)
        assert np.array_equal(fine['hist'][z], np.histogram(E[~np.isnan(E[:, 0]), 0], bins=fine['edges'])[0])
    for name in ref.NAMES:
        for k in STATS:
            assert np.array_equal(fine[name][k], got[name][k], equal_nan=True)


def test_sets_refuse_a_negative_weight(lib, sets_case):
    from bayhunter_amd import _lib, moho
    rows, D, w, start = sets_case
    w = w.copy()
    w[start[6] + 17] = -1
    with pytest.raises(_lib.BayHunterAmdError, match='negative weight'):
        moho.summarize_sets(rows, start, w, WINDOW, MOHOVS)
    with pytest.raises(_lib.BayHunterAmdError, match='negative weight'):
        moho.summarize(rows, w, WINDOW, MOHOVS)


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


def test_station_pool_moho_equals_every_station_views(station_pool):
    from bayhunter_amd.selection import pool_rows
    pool = station_pool
    for kw in (dict(selection='weighted'), dict(selection='saved'), dict(selection='weighted', exclude_outliers=False)):
        res = pool.moho(mohovs=POOL_MOHOVS, dev=0.5, **kw)
        assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and res.hist.shape == (3, 50)
        z = pool.pool.priors['z']
        assert np.array_equal(res.edges, np.linspace(z[0], z[1], 51))
        assert (res.nmodels > 0).any()
        for s, name in enumerate(res.names):
            if res.nmodels[s] == 0:
                with pytest.raises(ValueError):
                    pool.station(name).moho(mohovs=POOL_MOHOVS, dev=0.5, **kw)
                assert np.isnan(res.moho['median'][s])
                continue
            one = pool.station(name).moho(mohovs=POOL_MOHOVS, dev=0.5, **kw)
            assert res.nmodels[s] == one['nmodels'] and res.nexcluded[s] == one['nexcluded']
            assert res.fraction[s] == one['nmodels'] / float(one['nmodels'] + one['nexcluded'])
            for q in ref.NAMES:
                for k in ('median', 'min', 'max'):
                    assert getattr(res, q)[k][s] == one[q][k], (name, q, k)
                np.testing.assert_allclose(getattr(res, q)['mean'][s], one[q]['mean'], rtol=MEAN_RTOL, atol=0)
                np.testing.assert_allclose(getattr(res, q)['std'][s], one[q]['std'], rtol=STD_RTOL, atol=STD_ATOL)
            assert res.hist[s].sum() == one['nmodels']
            # the station's histogram: numpy's over the shared edges, from the restatement on the rows of its view
            view = pool.station(name)
            ci, ri, w = pool_rows(view, kw['selection'], 0.5, kw.get('exclude_outliers', True))
            D = ref.derive(view.models[ci, ri].astype(np.float64), z, POOL_MOHOVS)
            E = np.repeat(D[:, 0], w)
            assert np.array_equal(res.hist[s], np.histogram(E[~np.isnan(E)], bins=res.edges)[0]), name


def test_chain_pool_moho_of_the_saved_rows_equals_the_restatement(station_pool, tmp_path):
    view = station_pool.station('BBB')
    view.save(str(tmp_path))
    files = sorted(glob.glob(str(tmp_path / 'data' / 'c???_p2models.npy')))
    assert len(files) == 4
    models = np.concatenate([np.load(f) for f in files])
    assert models.dtype == np.float64 and view.models.dtype == np.float32         # save() widens, so does the pool
    z = view.priors['z']
    want = ref.summarize(models, None, z, POOL_MOHOVS)
    got = view.moho(mohovs=POOL_MOHOVS, selection='saved', exclude_outliers=False)
    assert np.array_equal(got['chains'], np.arange(4))
    assert_summary({k: v for k, v in got.items() if k != 'chains'}, want)
