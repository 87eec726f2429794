"""StationPool.datafits on the GPU: one forward pass and one segmented reduction for all stations against the loop over
the station views -- 5 stations x 3 short chains on the tutorial's two targets, every station its own receiver-function
slowness (per_station=('p',)), one station with gaps (missing='mask'), the stations taken in several runs (max_rows).
Bit identity is the criterion: first of the pooled forward matrix against the per-station matrices (the library's row
independence), then of every field of every station's dict."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
from chain_scenario import CASES  # noqa: E402
from station_scenario import make_stations  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, 'tutorial_observed')
NAMES = ['AAA', 'BBB', 'CCC', 'DDD', 'EEE']
PS = [4.5, 5.5, 6.5, 7.5, 8.5]
C_PER = 3


def _assert_equal_trees(a, b, path=''):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _assert_equal_trees(a[k], b[k], '%s/%s' % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_equal_trees(x, y, '%s[%d]' % (path, i))
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype, path
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind in 'fc' else np.array_equal(x, y), path


@pytest.fixture(scope='module')
def pool(lib):
    from bayhunter_amd.stations import StationPool
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=80, iter_main=40)
    st = make_stations(DATA, 5, yerr=True)
    for joint, p in zip(st, PS):
        joint.targets[1].moddata.plugin.set_modelparams(p=p)
    y = st[3].targets[0].obsdata.y.copy()                           # station DDD lacks two periods
    y[[2, 7]] = np.nan
    st[3].targets[0].obsdata.y = y
    with StationPool(dict(zip(NAMES, st)), ip, case['priors'], chains_per_station=C_PER, random_seeds=[3, 1, 4, 15, 9],
                     nmodels=121, per_station=('p',), missing='mask') as sp:
        sp.run()
    return sp


def test_pooled_forward_rows_equal_the_stations_own(pool):
    from bayhunter_amd.datafits import forward_matrix
    from bayhunter_amd.selection import station_rows
    from bayhunter_amd.stations import rf_slowness_table
    inner = pool.pool
    ci, ri, w, start, failed = station_rows(inner, C_PER, 'weighted', 0.5, True)
    assert not failed and np.all(np.diff(start) > 0)
    models, vpvs = inner.models[ci, ri], inner.vpvs[ci, ri].astype(np.float64)
    mantle = inner.priors.get('mantle')
    table = rf_slowness_table(pool.stations)
    assert np.array_equal(table[:, 0], PS)
    eng, Y, err, _ = forward_matrix(pool.stations[0], models, vpvs, mantle, rf_p=table,
                                    set_id=np.repeat(np.arange(5, dtype=np.int32), np.diff(start)))
    Y, err = Y[:, :eng.ncols].cpu().numpy(), err.cpu().numpy()
    rows = set()
    for s in range(5):
        a, b = start[s], start[s + 1]
        e1, Y1, err1, _ = forward_matrix(pool.stations[s], models[a:b], vpvs[a:b], mantle)
        assert Y[a:b].tobytes() == Y1[:, :e1.ncols].cpu().numpy().tobytes(), s
        assert np.array_equal(err[a:b], err1.cpu().numpy()), s
        rows.add(Y[a].tobytes())
    assert len(rows) == 5                                           # (every station's first row is its own)


def test_station_pool_datafits_equals_every_station_view(pool):
    from bayhunter_amd.datafits import station_runs
    from bayhunter_amd.selection import station_rows
    start = station_rows(pool.pool, C_PER, 'weighted', 0.5, True)[3]
    max_rows = int(np.diff(start).max()) + 1
    assert len(station_runs(start, max_rows)) >= 2
    res = pool.datafits(dev=0.5, nbins=40, max_rows=max_rows)
    one = pool.datafits(dev=0.5, nbins=40)                          # all stations in one run
    assert not res.failed and list(res.stations) == NAMES and res.names == NAMES
    _assert_equal_trees(one.stations, res.stations, 'runs')
    for s, name in enumerate(NAMES):
        want = pool.station(name).datafits(dev=0.5, nbins=40)
        _assert_equal_trees(res.stations[name], want, name)
        assert res.nmodels[s] == want['nmodels'] and res.nexcluded[s] == want['nexcluded']
        for t, d in enumerate(want['targets']):
            for k in res.FIELDS:
                assert np.array_equal(getattr(res, k)[t][s], d[k], equal_nan=True), (name, k)
            assert np.array_equal(res.quantiles[t][s], d['quantiles']), name
    gap = res.stations['DDD']['targets'][0]
    assert np.isnan(gap['yobs'][[2, 7]]).all() and np.isnan(gap['residual'][[2, 7]]).all()
    assert np.isfinite(np.delete(gap['residual'], [2, 7])).all() and np.isfinite(gap['best']).all()
    assert res.refs == [d['ref'] for d in want['targets']] and res.mean[0].shape == (5, gap['mean'].size)
    # other selections take the same path
    sv = pool.datafits(selection='saved', exclude_outliers=False, max_rows=max_rows)
    for name in NAMES:
        _assert_equal_trees(sv.stations[name], pool.station(name).datafits(selection='saved', exclude_outliers=False), name)


def test_a_failed_station_is_named(pool):
    """station BBB loses its main-phase rows: the others keep their results (this test runs last: it edits the pool)"""
    before = pool.datafits(dev=0.5, nbins=40)
    pool.pool.iter[C_PER:2 * C_PER] = -1
    with pytest.raises(ValueError, match="station 'BBB'.*empty selection"):
        pool.datafits(dev=0.5, nbins=40)
    res = pool.datafits(dev=0.5, nbins=40, strict=False)
    assert list(res.failed) == ['BBB'] and 'empty selection' in res.failed['BBB'] and list(res.stations) == NAMES[:1] + NAMES[2:]
    for name in res.stations:
        _assert_equal_trees(res.stations[name], before.stations[name], name)
    assert np.isnan(res.mean[0][1]).all() and np.isnan(res.quantiles[1][1]).all() and res.nmodels[1] == 0
    assert np.isfinite(res.mean[0][[0, 2, 3, 4]]).all()
