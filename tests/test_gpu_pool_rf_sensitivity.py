"""GPU tier of ChainPool.rf_sensitivity and StationPool.rf_sensitivity (bayhunter_amd/sensitivity.py): a pool of two
chains and a StationPool of 3 stations x 2 chains built with per_station=('p',), a few hundred iterations each, on the
first 64 samples of the tutorial's P receiver function and its Rayleigh phase velocities, at most 5 layers.

* ChainPool.rf_sensitivity() lies within the derived bounds (tests/rf_sens_sets_tolerances.py) of the numpy restatement
  sensitivity.rf_batch + vs_total + to_depth on the same rows, summed in longdouble on the expanded matrix; every model
  with two layers or more has a trace, so nexcluded == 0 and nmodels is the sum of the weights;
* t and every select cells of the full result; max_rows changes no bit;
* StationPool.rf_sensitivity() is, station by station, bit for bit what the station's view returns, and what
  rf_summarize returns for the station's rows at the station's own ray parameter -- not at another station's;
* the refusals; ForwardEngine.rf_sensitivity(p=...) equals an engine built with that p.

Worst error over bound as measured on one MI355X: see tests/rf_sens_sets_tolerances.py (WORST_POOL).
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import rf_sens_sets_tolerances as tol  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, 'tutorial_observed')
ARRAYS = ('mean', 'std', 'min', 'max', 'halfspace_mean', 'halfspace_std', 'nmodels', 'nexcluded')
NT = 64
P = [6.4, 7.4, 6.4]                 # the stations' ray parameters [s/deg]


def joint(refs=('rdispph', 'prf'), p=None, seed=None):
    """The tutorial's targets with the receiver functions cut to their first NT samples; y perturbed by `seed`."""
    from bayhunter_amd import targets as T
    from chain_scenario import target_classes
    out = []
    for ref in refs:
        d = np.loadtxt(os.path.join(DATA, 'st3_%s.dat' % ref))
        if ref in ('prf', 'srf'):
            d = d[:NT]
        y = d[:, 1]
        if seed is not None:
            y = y + (0.005 if ref in ('prf', 'srf') else 0.02) * np.random.RandomState(seed).standard_normal(y.size)
        t = target_classes(T)[ref](d[:, 0], y)
        if p is not None and ref in ('prf', 'srf'):
            t.moddata.plugin.set_modelparams(p=p)
        out.append(t)
    return T.JointTarget(out)


def params(burnin, main):
    from chain_scenario import CASES
    case = CASES['tutorial']
    return dict(case['initparams'], iter_burnin=burnin, iter_main=main), dict(case['priors'], layers=(1, 5))


@pytest.fixture(scope='module')
def chain_pool(lib):
    from bayhunter_amd.chains import ChainPool, GpuEvaluator
    ip, priors = params(150, 200)
    j = joint()
    return ChainPool(j, initparams=ip, modelpriors=priors, seeds=[41, 42], evaluator=GpuEvaluator(j)).run()


@pytest.fixture(scope='module')
def station_pool(lib):
    from bayhunter_amd.stations import StationPool
    ip, priors = params(150, 200)
    stations = [joint(p=P[s], seed=None if s == 0 else 2024 + s) for s in range(3)]
    with StationPool(dict(zip(['AAA', 'BBB', 'CCC'], stations)), ip, priors, chains_per_station=2,
                     random_seeds=[51, 52, 53], nmodels=351, per_station=('p',)) as pool:
        pool.run()
    return pool


def same_result(one, other):
    assert sorted(one) == sorted(other)
    for k in one:
        a, b = np.asarray(one[k]), np.asarray(other[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def restatement(pool, ci, ri, spec, edges):
    """Per row the binned kernel from sensitivity.rf_batch + vs_total + to_depth -> (x, a [rows, nt, bins + 1] float64 with
    the half-space last -- a the same from the magnitudes of K --, nlay [rows], rf [rows, nt], Lmax)."""
    import torch
    from bayhunter_amd import datafits as df, sensitivity as sens
    from bayhunter_amd.models import layers_from_voronoi
    rows = torch.from_numpy(pool.models[ci, ri].astype(np.float64)).cuda()
    vsn, zv, nl = df._layers(rows, rows.device)
    dm, _ = layers_from_voronoi(vsn, zv, nl, torch.from_numpy(pool.vpvs[ci, ri].astype(np.float64)).cuda(), df._OPEN_PRIORS,
                                mantle=pool.priors.get('mantle'))
    H, VP, VS, RHO = (dm.packed[:, k, :].cpu().numpy() for k in range(4))
    nlay = dm.nlay.cpu().numpy()
    par = dict(obsx=spec.obsx, gauss=spec.gauss, p=spec.p, nsv=spec.nsv, wtype={0: 'P', 1: 'SV'}[spec.waveno])
    res = sens.rf_batch(par, H, VP, VS, RHO, nlay, spec.ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        G = sens.vs_total(res['K'], (VP / VS)[:, None, :])
        Ga = sens.vs_total(np.abs(res['K']), (VP / VS)[:, None, :])
    x, a = np.zeros((ci.size, spec.obsx.size, edges.size)), np.zeros((ci.size, spec.obsx.size, edges.size))
    for r in range(ci.size):
        n = int(nlay[r])
        if n >= 2:
            x[r, :, :-1], x[r, :, -1] = sens.to_depth(G[r][:, :n], H[r, :n], edges)
            a[r, :, :-1], a[r, :, -1] = sens.to_depth(Ga[r][:, :n], H[r, :n], edges)
    return x, a, nlay, res['rf'], H.shape[1]


def test_chain_pool_rf_sensitivity_lies_within_the_bounds_of_the_restatement(chain_pool):
    from bayhunter_amd import sensitivity as sens
    from bayhunter_amd.selection import pool_rows
    pool = chain_pool
    assert pool.maxlayers <= 6
    got = pool.rf_sensitivity(dev=0.5)
    spec, _ = sens.pool_rf_target(pool.targets)
    edges = got['edges']
    assert spec.obsx.size == NT and np.array_equal(edges, sens.default_edges()) and got['kind'] == 'vs_total'
    assert got['ref'] == 'prf' and got['mean'].shape == (NT, 100) and got['halfspace_std'].shape == (NT,)
    assert np.array_equal(got['samples'], np.arange(NT)) and np.allclose(got['t'], pool.targets.targets[1].obsdata.x)
    ci, ri, w = pool_rows(pool, 'weighted', 0.5, True)
    assert np.array_equal(got['chains'], np.unique(ci) + pool.first)
    x, a, nlay, rf, Lmax = restatement(pool, ci, ri, spec, edges)
    counts = (w > 0) & (nlay >= 2) & ~np.isnan(rf[:, 0])
    assert not np.isnan(rf[nlay >= 2, 0]).any()                      # every model with two layers or more has a trace
    assert isinstance(got['nmodels'], int) and got['nexcluded'] == 0 and got['nmodels'] == w[counts].sum() == w.sum() > 0
    rows = np.nonzero(counts)[0]
    LD = np.longdouble
    wl, X, A = w[rows].astype(LD)[:, None, None], x[rows].astype(LD), a[rows].astype(LD)
    W = wl.sum()
    mean, sq = (wl * X).sum(axis=0) / W, (wl * X * X).sum(axis=0) / W
    a1, a2 = (wl * A).sum(axis=0) / W, (wl * A * A).sum(axis=0) / W
    gm = np.concatenate([got['mean'], got['halfspace_mean'][:, None]], axis=1)
    gs = np.concatenate([got['std'], got['halfspace_std'][:, None]], axis=1)
    worst = []
    for err, bound in ((np.abs(gm - mean), tol.mean_bound(rows.size, Lmax, a1)),
                       (np.abs(gs.astype(LD) ** 2 - (sq - mean * mean)), tol.var_bound(rows.size, Lmax, a2))):
        err = err.astype(np.float64)
        worst.append(float(np.where(err == 0, 0., err / np.where(err == 0, 1., bound)).max()))
    print('worst error / bound: mean %.3g, variance %.3g' % tuple(worst))
    assert worst[0] <= 1. and worst[1] <= 1., worst
    scale = np.abs(x[rows][:, :, :-1]).max()
    assert np.allclose(got['min'], x[rows][:, :, :-1].min(axis=0), rtol=1e-9, atol=1e-12 * scale)
    assert np.allclose(got['max'], x[rows][:, :, :-1].max(axis=0), rtol=1e-9, atol=1e-12 * scale)
    assert np.abs(got['mean']).max() > 0 and (got['std'] >= 0).all()
    # t and every select cells of the full result; max_rows changes no bit
    t = got['t']
    part = pool.rf_sensitivity(dev=0.5, t=(t[10], t[40]), every=3)
    idx = np.arange(10, 41)[::3]
    assert np.array_equal(part['samples'], idx) and np.array_equal(part['t'], t[idx])
    for k in ('mean', 'std', 'min', 'max', 'halfspace_mean', 'halfspace_std'):
        assert part[k].tobytes() == np.ascontiguousarray(got[k][idx]).tobytes(), k
    assert part['nmodels'] == got['nmodels']
    same_result(pool.rf_sensitivity(dev=0.5, max_rows=1), got)
    small = pool.rf_sensitivity(dep_edges=[0., 10., 35., 70.], kind='vs', selection='saved', dev=0.5, every=7)
    assert small['mean'].shape == (10, 3) and small['kind'] == 'vs'


def test_station_pool_rf_sensitivity_equals_every_station_view_at_its_own_p(station_pool):
    from bayhunter_amd import sensitivity as sens
    from bayhunter_amd.selection import station_rows
    pool = station_pool
    res = pool.rf_sensitivity(dev=0.5, every=2)
    assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and sorted(res.stations) == res.names
    S = NT // 2
    assert res.mean.shape == res.std.shape == res.min.shape == res.max.shape == (3, S, 100) and res.t.shape == (S,)
    assert res.halfspace_mean.shape == (3, S) and res.nmodels.shape == res.nexcluded.shape == (3,) and res.ref == 'prf'
    assert np.array_equal(res.p, P)
    runs = pool.rf_sensitivity(dev=0.5, every=2, max_rows=1)
    ci, ri, w, set_start, _ = station_rows(pool.pool, 2, 'weighted', 0.5, True)
    inner = pool.pool
    for s, name in enumerate(res.names):
        view = pool.station(name)
        one = view.rf_sensitivity(dev=0.5, every=2)                    # ChainPool.rf_sensitivity on the station's view
        same_result(res.stations[name], one)
        same_result(runs.stations[name], one)                           # no result depends on the runs
        assert one['nmodels'] > 0 and one['nexcluded'] == 0 and np.all(one['min'] <= one['max'])
        for k in ARRAYS:
            assert np.asarray(getattr(res, k)[s]).tobytes() == np.asarray(one[k]).tobytes(), (name, k)
        # the station's rows at the station's own ray parameter, and not at another's
        spec, _ = sens.pool_rf_target(view.targets)
        assert spec.p == P[s]
        a, b = set_start[s], set_start[s + 1]
        rows, vpvs, ws = inner.models[ci[a:b], ri[a:b]], inner.vpvs[ci[a:b], ri[a:b]].astype(np.float64), w[a:b].astype(np.int32)
        par = dict(obsx=spec.obsx, gauss=spec.gauss, nsv=spec.nsv)
        own = sens.rf_summarize(dict(par, p=P[s]), rows, vpvs, ws, every=2, mantle=inner.priors.get('mantle'))
        for k in own:                                                   # (the pool's dict has 'ref' and 'chains' besides)
            assert np.asarray(own[k]).tobytes() == np.asarray(one[k]).tobytes(), (name, k)
        other = sens.rf_summarize(dict(par, p=P[(s + 1) % 3] if P[(s + 1) % 3] != P[s] else P[1]), rows, vpvs, ws, every=2,
                                  mantle=inner.priors.get('mantle'))
        assert other['nmodels'] == one['nmodels'] and not np.array_equal(other['mean'], one['mean'])
    assert not np.array_equal(res.mean[0], res.mean[1])


def test_refusals(chain_pool):
    from bayhunter_amd import sensitivity as sens
    from bayhunter_amd.chains import ChainPool, GpuEvaluator
    pool = chain_pool
    with pytest.raises(ValueError, match="no receiver-function target 'srf'"):
        pool.rf_sensitivity(ref='srf')
    with pytest.raises(ValueError, match='no receiver-function target'):
        pool.rf_sensitivity(ref='rdispph')
    with pytest.raises(ValueError, match='no sample'):
        pool.rf_sensitivity(t=(1e3, 2e3))
    with pytest.raises(ValueError, match='every'):
        pool.rf_sensitivity(every=0)
    with pytest.raises(ValueError, match='kind'):
        pool.rf_sensitivity(kind='h')
    ip, priors = params(10, 10)
    for refs, match in ((('rdispph',), 'the pool has no receiver-function target'), (('rdispph', 'prf', 'srf'), "ref is one of 'prf', 'srf'")):
        j = joint(refs)
        with ChainPool(j, initparams=ip, modelpriors=priors, seeds=[1, 2], evaluator=GpuEvaluator(j)) as other:
            with pytest.raises(ValueError, match=match):
                other.rf_sensitivity()
    with pytest.raises(ValueError, match='p: a number, or one per set'):
        sens.rf_summarize_sets(dict(obsx=np.arange(NT) * 0.2 - 5.), np.zeros((4, 10)), [0, 2, 4], 1.73, p=[6., 7., 8.])


def test_engine_rf_sensitivity_takes_a_ray_parameter_for_the_call(lib):
    import torch
    from bayhunter_amd.engine import ForwardEngine, RfSpec
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(40, 6, seed=3)
    obsx = np.arange(NT) * 0.2 - 5.
    a, b = ForwardEngine(rf=[RfSpec('prf', obsx, 1.0, 6.4)]), ForwardEngine(rf=[RfSpec('prf', obsx, 1.0, 7.4)])
    ma, mb = a.upload(H, VP, VS, RHO, nl), b.upload(H, VP, VS, RHO, nl)
    plain, want = a.rf_sensitivity(ma), b.rf_sensitivity(mb)
    got = a.rf_sensitivity(ma, p=7.4)
    again = a.rf_sensitivity(ma)                                    # the engine keeps its own
    torch.cuda.synchronize()
    for k in ('K', 'rf'):
        g, w_, p0, p1 = (v[k].cpu().numpy() for v in (got, want, plain, again))
        assert g.tobytes() == w_.tobytes() and p0.tobytes() == p1.tobytes() and g.tobytes() != p0.tobytes(), k
    assert a.rf[0].p == 6.4 and a._rfp[0].p == 6.4
