"""GPU tier of ChainPool.sensitivity and StationPool.sensitivity (bayhunter_amd/sensitivity.py): a tutorial pool of six
chains and a StationPool of 3 stations x 2 chains, a few hundred iterations each.

* ChainPool.sensitivity() lies within the derived bounds (tests/sens_sets_tolerances.py) of the numpy restatement
  sensitivity.batch + vs_total + to_depth on the same rows, summed in longdouble on the expanded matrix;
* StationPool.sensitivity() is, station by station, bit for bit what the station's view returns;
* max_rows = 300 (sets cut at block multiples, several add calls) changes no bit;
* a pool whose only dispersion target is a group-velocity target is refused.

Worst error over bound as measured on one MI355X: mean 0.010, variance 0.020.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import sens_sets_tolerances as tol  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, 'tutorial_observed')
ARRAYS = ('mean', 'std', 'min', 'max', 'halfspace_mean', 'halfspace_std', 'nmodels', 'nexcluded')


@pytest.fixture(scope='module')
def chain_pool(lib):
    from bayhunter_amd.chains import GpuEvaluator
    from chain_scenario import CASES, make_pool
    case = dict(CASES['tutorial'], burnin=200, main=300)
    return make_pool(None, DATA, case, seeds=list(range(41, 47)), evaluator=GpuEvaluator).run()


@pytest.fixture(scope='module')
def station_pool(lib):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=150, iter_main=300)
    stations = make_stations(DATA, 3, refs=case.get('refs', ('rdispph', 'prf')), yerr=True)
    with StationPool(dict(zip(['AAA', 'BBB', 'CCC'], stations)), ip, case['priors'], chains_per_station=2,
                     random_seeds=[51, 52, 53], nmodels=451) as pool:
        pool.run()
    return pool


def same_result(one, other):
    assert sorted(one) == sorted(other)
    for k in one:
        a, b = np.asarray(one[k]), np.asarray(other[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def restatement(pool, ci, ri, w, periods, edges):
    """Per row the binned kernel from sensitivity.batch + vs_total + to_depth -> (x [rows, nper, bins + 1] float64 with
    the half-space last, counts [rows, nper], Lmax)."""
    import torch
    from bayhunter_amd import datafits as df, sensitivity as sens
    from bayhunter_amd.models import layers_from_voronoi
    rows = torch.from_numpy(pool.models[ci, ri].astype(np.float64)).cuda()
    vsn, zv, nl = df._layers(rows, rows.device)
    dm, _ = layers_from_voronoi(vsn, zv, nl, torch.from_numpy(pool.vpvs[ci, ri].astype(np.float64)).cuda(), df._OPEN_PRIORS,
                                mantle=pool.priors.get('mantle'))
    H, VP, VS, RHO = (dm.packed[:, k, :].cpu().numpy() for k in range(4))
    nlay = dm.nlay.cpu().numpy()
    res = sens.batch(periods, H, VP, VS, RHO, nlay, 'rayleigh')
    with np.errstate(invalid='ignore', divide='ignore'):
        G = sens.vs_total(res['K'], (VP / VS)[:, None, :])
    x = np.zeros((ci.size, periods.size, edges.size))
    for r in range(ci.size):
        n = int(nlay[r])
        if n >= 2:
            x[r, :, :-1], x[r, :, -1] = sens.to_depth(G[r][:, :n], H[r, :n], edges)
    return x, (w > 0)[:, None] & (nlay >= 2)[:, None] & ~np.isnan(res['c']), H.shape[1]


def test_chain_pool_sensitivity_lies_within_the_bounds_of_the_restatement(chain_pool):
    from bayhunter_amd import sensitivity as sens
    from bayhunter_amd.selection import pool_rows
    pool = chain_pool
    got = pool.sensitivity(dev=0.5)
    periods, edges = got['periods'], got['edges']
    assert np.array_equal(periods, pool.targets.targets[0].obsdata.x) and np.array_equal(edges, sens.default_edges())
    assert got['kind'] == 'vs_total' and got['ref'] == 'rdispph' and got['mean'].shape == (periods.size, 100)
    ci, ri, w = pool_rows(pool, 'weighted', 0.5, True)
    assert np.array_equal(got['chains'], np.unique(ci) + pool.first)
    x, counts, Lmax = restatement(pool, ci, ri, w, periods, edges)
    LD = np.longdouble
    worst = [0., 0.]
    for p in range(periods.size):
        rows = np.nonzero(counts[:, p])[0]
        assert got['nmodels'][p] == w[rows].sum() > 0 and got['nexcluded'][p] == w.sum() - w[rows].sum()
        wl, X = w[rows].astype(LD)[:, None], x[rows, p, :].astype(LD)
        W = wl.sum()
        mean, sq, ab = (wl * X).sum(axis=0) / W, (wl * X * X).sum(axis=0) / W, (wl * np.abs(X)).sum(axis=0) / W
        gm = np.r_[got['mean'][p], got['halfspace_mean'][p]]
        gs = np.r_[got['std'][p], got['halfspace_std'][p]]
        n = np.array([rows.size])
        for i, (err, bound) in enumerate(((np.abs(gm - mean), tol.mean_bound(n, Lmax, ab[None, :])[0]),
                                          (np.abs(gs.astype(LD) ** 2 - (sq - mean * mean)), tol.var_bound(n, Lmax, sq[None, :])[0]))):
            err = err.astype(np.float64)
            worst[i] = max(worst[i], float(np.where(err == 0, 0., err / np.where(err == 0, 1., bound)).max()))
        # (min and max are the device's own cells: to_depth's matrix product rounds otherwise)
        scale = np.abs(x[rows, p, :-1]).max()
        assert np.allclose(got['min'][p], x[rows, p, :-1].min(axis=0), rtol=1e-9, atol=1e-12 * scale)
        assert np.allclose(got['max'][p], x[rows, p, :-1].max(axis=0), rtol=1e-9, atol=1e-12 * scale)
    print('worst error / bound: mean %.3g, variance %.3g' % tuple(worst))
    assert worst[0] <= 1. and worst[1] <= 1., worst
    # the data look into the crust at short periods and deeper at long ones
    depth = lambda p: np.nansum(np.abs(got['mean'][p]) * 0.5 * (edges[1:] + edges[:-1])) / np.nansum(np.abs(got['mean'][p]))
    assert depth(0) < depth(periods.size - 1)
    # the other kinds, an edge grid of one's own, the saved selection; max_rows changes no bit
    small = pool.sensitivity(dep_edges=[0., 10., 35., 70.], kind='vs', selection='saved', dev=0.5)
    assert small['mean'].shape == (periods.size, 3) and small['kind'] == 'vs'
    same_result(pool.sensitivity(dev=0.5, max_rows=300), got)
    with pytest.raises(ValueError, match='no dispersion target'):
        pool.sensitivity(ref='ldispph')


def test_station_pool_sensitivity_equals_every_station_view(station_pool):
    pool = station_pool
    res = pool.sensitivity(dev=0.5)
    assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and sorted(res.stations) == res.names
    P = res.periods.size
    assert res.mean.shape == res.std.shape == res.min.shape == res.max.shape == (3, P, 100)
    assert res.halfspace_mean.shape == res.nmodels.shape == res.nexcluded.shape == (3, P) and res.ref == 'rdispph'
    runs = pool.sensitivity(dev=0.5, max_rows=300)
    for s, name in enumerate(res.names):
        one = pool.station(name).sensitivity(dev=0.5)                   # ChainPool.sensitivity on the station's view
        same_result(res.stations[name], one)
        same_result(runs.stations[name], one)                          # no result depends on the runs
        assert one['nmodels'].min() > 0 and np.all(one['min'] <= one['max']) and np.all(one['std'] >= 0)
        for k in ARRAYS:
            assert getattr(res, k)[s].tobytes() == one[k].tobytes(), (name, k)
    assert not np.array_equal(res.mean[0], res.mean[1])


def test_a_station_without_rows_is_nan_and_a_group_velocity_pool_is_refused(station_pool):
    pool = station_pool
    inner = pool.pool
    keep = inner.iter[4:6].copy()
    inner.iter[4:6] = -1                                    # station CCC: no main-phase row
    try:
        res = pool.sensitivity(dev=0.5)
        assert list(res.failed) == ['CCC'] and sorted(res.stations) == ['AAA', 'BBB']
        assert np.isnan(res.mean[2]).all() and np.isnan(res.halfspace_std[2]).all() and not res.nmodels[2].any()
        assert not np.isnan(res.mean[:2]).all()
        with pytest.raises(ValueError, match="station 'CCC'"):
            pool.sensitivity(dev=0.5, strict=True)
        with pytest.raises(ValueError, match='empty selection'):
            pool.station('CCC').sensitivity(dev=0.5)
    finally:
        inner.iter[4:6] = keep
    from bayhunter_amd.chains import GpuEvaluator
    from chain_scenario import CASES, make_pool
    with make_pool(None, DATA, dict(CASES['tutorial'], refs=('rdispgr', 'prf'), burnin=20, main=10), seeds=[1, 2],
                   evaluator=GpuEvaluator) as group:
        with pytest.raises(ValueError, match='group-velocity targets are not served'):
            group.sensitivity()
