"""GPU tier of the convergence diagnostics (bh_autocov_sets, bayhunter_amd/convergence.py, ChainPool.convergence,
StationPool.convergence) against the host twin (tests/hostsim/autocov_sim.cpp: bit for bit) and the numpy restatement
(tests/convergence_ref.py: within tests/convergence_tolerances.py, and what that bound propagates to)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import convergence_ref as ref  # noqa: E402
from convergence_tolerances import check_acov, input_bounds, propagate  # noqa: E402
from test_convergence import load_sim, plan, sim  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def asim():
    return load_sim()


def autocov(D, w, start, mean, nlags, pad=0, expect=0):
    """bh_autocov_sets over the host matrix D (uploaded, `pad` unused columns of 7.0 beyond it) -> (acov, length), or
    the error text."""
    import torch
    from bayhunter_amd import _lib
    lib = _lib.load()
    R, K = D.shape
    t = torch.full((R, K + pad), 7.0, dtype=torch.float64, device='cuda')
    t[:, :K] = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float64)).cuda()
    dw = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.int32)).cuda()
    start = np.ascontiguousarray(start, dtype=np.int64)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    S = start.size - 1
    acov = np.full((S, K, nlags), -7.)
    length = np.full(S, -1, dtype=np.int64)
    rc = lib.bh_autocov_sets(t.data_ptr(), R, K + pad, K, None if dw is None else dw.data_ptr(), start.ctypes.data, S,
                             mean.ctypes.data, nlags, acov.ctypes.data, length.ctypes.data,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == expect, lib.bh_last_error()
    return (acov, length) if rc == 0 else lib.bh_last_error().decode()


def series_set(T, nlags, weighted):
    """About 40 series of 5 columns: the CPU tier's lengths three times over with other values."""
    parts = [ref.series_case(T, nlags, seed=s, weighted=weighted) for s in (11, 12, 13)]
    D = np.concatenate([p[0] for p in parts])
    w = np.concatenate([p[1] for p in parts]) if weighted else None
    start, lengths = [0], []
    for p in parts:
        start += (p[2][1:] + start[-1]).tolist()
        lengths += p[3].tolist()
    return D, w, np.asarray(start, dtype=np.int64), np.asarray(lengths, dtype=np.int64)


@pytest.mark.parametrize('weighted', [True, False])
@pytest.mark.parametrize('nlags', [1, 2, 3, 64, 65, 257, 4096])
def test_autocov_sets_equals_the_twin_bit_for_bit(lib, asim, nlags, weighted):
    _, T = plan(asim, nlags)
    D, w, start, lengths = series_set(T, nlags, weighted)
    assert 36 <= lengths.size <= 42 and D.shape[1] == 5
    mean = ref.series_means(D, w, start)
    got, glen = autocov(D, w, start, mean, nlags, pad=3)
    assert np.array_equal(glen, lengths)
    twin, _ = sim(asim, D, w, start, mean, nlags)
    assert ref.same(got, twin)
    again, _ = autocov(D, w, start, mean, nlags)                   # two runs, and no stride in the result
    assert got.tobytes() == again.tobytes()
    if nlags <= 257 or weighted:                                    # (the restatement at 4096 lags once)
        want, length, absprod = ref.autocov(D, w, start, mean, nlags)
        print('nlags %d: worst |difference| / bound %.3f' % (nlags, check_acov(got, want, lengths, absprod)))


def test_a_nan_stays_in_its_column_and_a_negative_weight_is_refused(lib, asim):
    from bayhunter_amd import _lib
    nlags = 65
    _, T = plan(asim, nlags)
    D, w, start, lengths = series_set(T, nlags, True)
    mean = ref.series_means(D, w, start)
    got, _ = autocov(D, w, start, mean, nlags)
    s = int(np.argmax(lengths))
    D2 = D.copy()
    D2[start[s] + np.nonzero(w[start[s]:start[s + 1]] > 0)[0][700], 2] = np.nan
    got2, _ = autocov(D2, w, start, mean, nlags)
    twin2, _ = sim(asim, D2, w, start, mean, nlags)
    assert ref.same(got2, twin2) and np.isnan(got2[s, 2]).all()
    keep = np.ones(got.shape, dtype=bool)
    keep[s, 2] = False
    assert ref.same(got2[keep], got[keep])
    bad = w.copy()
    bad[start[s] + 17] = -1
    assert 'negative weight' in autocov(D, bad, start, mean, nlags, expect=_lib.BH_ERR_ARG)


def test_sixteen_columns_at_4096_lags_come_in_lag_groups(lib, asim):
    nlags = 4096
    _, T = plan(asim, nlags)
    rs = np.random.RandomState(14)
    n = 3 * T + 7
    w = rs.randint(0, 4, 2 * n).astype(np.int32)
    w = w[:np.searchsorted(np.cumsum(w), n) + 1]
    w[-1] -= w.sum() - n
    assert w.sum() == n and w.min() >= 0
    D = rs.randn(w.size, 16) * np.arange(1, 17)
    start = np.array([0, w.size], dtype=np.int64)
    mean = ref.series_means(D, w, start)
    got, glen = autocov(D, w, start, mean, nlags)
    twin, _ = sim(asim, D, w, start, mean, nlags)
    assert glen[0] == n and ref.same(got, twin)
    want, length, absprod = ref.autocov(D[:, :2], w, start, mean[:, :2], nlags)
    check_acov(got[:, :2], want, glen, absprod, 'two of sixteen columns')
    assert np.all(got[0, :, 0] > 0) and np.abs(got[0, :, 2048:]).max() > 0      # the second group of lags is there


# ---- the statistic ------------------------------------------------------------------------------------------

def test_summarize_on_the_four_ar1_sets(lib, asim):
    """Against the restatement within the bound of the autocovariances (and of the means) carried through the rules to
    first order (convergence_tolerances.propagate); against the rules on the twin's autocovariances exactly."""
    import torch
    from bayhunter_amd import convergence as cv, datafits as df, scalars
    for name, D, w, start, n, nlags in ref.ar1_sets():
        D = np.concatenate((D, 3. * D - 1.), axis=1)                 # a second column: the same chains, rescaled
        res = cv.summarize(scalars.Columns(D, ['f8', 'f8'], ['x', 'y']), w, start, [0, 8], nlags=nlags)
        assert not res.failed and len(res) == 1 and res[0]['n'] == n and res[0]['nseries'] == 8
        mean = ref.series_means(D, w, start)
        want_acov, length, absprod = ref.autocov(D, w, start, mean, nlags)
        for c, col in enumerate(('x', 'y')):
            got = res[0][col]
            want = ref.diagnose(mean[:, c], want_acov[:, c], n)
            dm, da = input_bounds(mean[:, c], absprod[:, c], n)
            tol = propagate(lambda m, a: ref.diagnose(m, a, n), mean[:, c], want_acov[:, c], dm, da, ('rhat', 'tau', 'ess'))
            print(name, col, {k: (got[k], want[k], tol[k]) for k in tol})
            assert got['truncated'] == want['truncated'] and not got['constant']
            for k in tol:
                assert abs(got[k] - want[k]) <= tol[k], (name, col, k)
        # exactly the rules on the twin: the means are the device's reduction, so the twin is handed the same ones
        M = torch.from_numpy(D).cuda()
        with df._FitsSets(M, 2, torch.from_numpy(w).cuda(), None, start, torch.cuda.current_stream().cuda_stream) as f:
            dmean = f.scan()['mean']
        twin, _ = sim(asim, D, w, start, dmean, nlags)
        exact = cv.group_diagnostics(dmean, twin, n, ['x', 'y'])
        for col in ('x', 'y'):
            for k in cv.FIELDS + ('acf', 'tau_chain', 'ess_chain'):
                assert ref.same(res[0][col][k], exact[col][k]), (name, col, k)
    with pytest.raises(ValueError, match='differ in length'):
        cv.summarize(scalars.Columns(D, ['f8', 'f8'], ['x', 'y']), w, np.r_[start[:-2], start[-1]], [0, 7], nlags=8)


# ---- pools --------------------------------------------------------------------------------------------------

def vs_at_depths(models, depths):
    """The Vs of the layer of posterior.stepmodel's step function that holds each depth, row by row: its depths come in
    pairs (top, bottom) per layer; a depth on an interface belongs to the layer below.  (stepmodel's interfaces are a
    cumulative sum of thicknesses and may differ from the midpoints in the last bit: the pool's depths 5 and 30 lie on
    no interface.)"""
    from bayhunter_amd.posterior import stepmodel
    out = np.empty((models.shape[0], len(depths)))
    for r, row in enumerate(models):
        vs, dep = stepmodel(row)
        bottoms = dep[1::2]
        for j, z in enumerate(depths):
            assert not np.any(np.abs(bottoms - z) < 1e-9)
            out[r, j] = vs[2 * np.searchsorted(bottoms, z, side='right')]
    return out


def restate_pool(view, chains, depths, nlags):
    """The restatement fed with pool.weighted(i)[2]: per column (diagnose's dict, its first-order tolerances), n, window."""
    nt = view.ntargets
    first, cols = {}, {}
    for i in chains:
        it = view.chain(i)['iter']
        first[i] = int(it[it >= 0][0])
        models, likes, misfits, noise, vpvs = view.weighted(i)[2]
        layers = (~np.isnan(models)).sum(axis=1) / 2 - 1
        cols[i] = np.column_stack([likes.astype(np.float64), misfits, vpvs.astype(np.float64), noise, layers] +
                                  ([vs_at_depths(models, depths)] if depths else []))
    t0 = max(first.values())
    n = (view.iter_main - t0) // 2
    series = []
    for i in chains:
        for lo, hi in ((view.iter_main - 2 * n, view.iter_main - n), (view.iter_main - n, view.iter_main)):
            series.append(cols[i][lo - first[i]:hi - first[i]])
    D = np.concatenate(series)
    start = np.arange(len(series) + 1) * n
    mean = ref.series_means(D, None, start)
    acov, _, absprod = ref.autocov(D, None, start, mean, min(nlags, 4096))
    out = []
    for c in range(D.shape[1]):
        d = ref.diagnose(mean[:, c], acov[:, c], n)
        keys = ('W', 'B', 'var_plus', 'mean') + (('rhat', 'tau', 'ess') if d['W'] > 0 else ())
        if d['W'] == 0:                      # a constant column: every y is exactly 0 on both sides
            out.append((d, dict.fromkeys(keys, 0.)))
            continue
        dm, da = input_bounds(mean[:, c], absprod[:, c], n)
        out.append((d, propagate(lambda m, a: ref.diagnose(m, a, n), mean[:, c], acov[:, c], dm, da, keys)))
    return out, n, (view.iter_main - 2 * n, view.iter_main)


@pytest.fixture(scope='module')
def station_pool(lib):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=150, iter_main=300)
    names = ['AAA', 'BBB', 'CCC', 'DDD', 'EEE']
    stations = make_stations(os.path.join(GOLDEN, 'tutorial_observed'), 5, refs=case.get('refs', ('rdispph', 'prf')), yerr=True)
    with StationPool(dict(zip(names, stations)), ip, case['priors'], chains_per_station=4,
                     random_seeds=[21, 22, 23, 24, 25], nmodels=451) as pool:
        pool.run()
    return pool


@pytest.fixture(scope='module')
def chain_pool(lib):
    from bayhunter_amd.chains import GpuEvaluator
    from chain_scenario import CASES, make_pool
    case = dict(CASES['tutorial'], burnin=200, main=300)
    return make_pool(None, os.path.join(GOLDEN, 'tutorial_observed'), case, seeds=list(range(31, 39)),
                     evaluator=GpuEvaluator).run()


@pytest.mark.parametrize('exclude', [True, False])
def test_chain_pool_convergence_equals_the_restatement(chain_pool, exclude):
    from bayhunter_amd import scalars
    from bayhunter_amd.selection import pool_rows
    view = chain_pool
    depths, nlags, dev = (5., 30.), 64, 0.5
    got = view.convergence(nlags=nlags, depths=depths, dev=dev, exclude_outliers=exclude)
    chains = np.unique(pool_rows(view, 'weighted', dev, exclude)[0])
    want, n, window = restate_pool(view, chains, depths, nlags)
    refs = [t.ref for t in view.targets.targets]
    names = scalars.NAMES(2, refs) + ['vs@5', 'vs@30']
    assert [k for k, v in got.items() if isinstance(v, dict)] == names
    assert got['n'] == n and got['window'] == window and got['nseries'] == 2 * chains.size
    assert np.array_equal(got['chains'], chains) and got['first_iter'].shape == chains.shape
    assert exclude or chains.size == 8
    for name, (w, tol) in zip(names, want):
        g = got[name]
        print(name, g['rhat'], w['rhat'], g['tau'], w['tau'], g['ess'], w['ess'], g['truncated'], g['constant'], tol)
        assert g['constant'] == w['constant'] and g['truncated'] == w['truncated']
        for k in ('W', 'B', 'var_plus', 'mean', 'rhat', 'tau', 'ess'):
            if k in tol:                     # the autocovariances' bound carried through the rules to first order
                assert abs(g[k] - w[k]) <= tol[k], (name, k, g[k], w[k], tol[k])
            else:
                assert np.isnan(g[k]) and np.isnan(w[k]), (name, k)
        assert g['converged'] == bool(g['rhat'] <= 1.01 and g['ess'] >= 100 * chains.size and not g['truncated'])
        assert g['tau_chain'].shape == g['ess_chain'].shape == chains.shape and g['acf'].shape == (nlags,)


def same_station(a, b):
    from bayhunter_amd import convergence as cv
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], dict):
            assert list(a[k]) == list(b[k])
            for f in a[k]:
                assert ref.same(a[k][f], b[k][f]), (k, f)
        else:
            assert np.array_equal(a[k], b[k]), k


def test_station_pool_convergence_equals_every_station_view(station_pool):
    pool = station_pool
    kw = dict(nlags=128, depths=(30.,), dev=0.5)
    res = pool.convergence(**kw)
    assert res.names == ['AAA', 'BBB', 'CCC', 'DDD', 'EEE'] and not res.failed and sorted(res.stations) == res.names
    assert res.columns[-1] == 'vs@30' and res.columns[0] == 'like' and res.window.shape == (5, 2)
    for s, name in enumerate(res.names):
        one = pool.station(name).convergence(**kw)
        same_station(res.stations[name], one)
        assert tuple(res.window[s]) == one['window']
        for c in res.columns:
            for f in ('rhat', 'ess', 'tau'):
                assert ref.same(getattr(res, f)[c][s], one[c][f]), (name, c, f)
            assert res.truncated[c][s] == one[c]['truncated'] and res.converged[c][s] == one[c]['converged']
    # runs of whole stations: no result depends on them
    hs_rows = sum(r['n'] for r in res.stations.values())
    split = pool.convergence(max_rows=max(1, hs_rows // 4), **kw)
    for name in res.names:
        same_station(split.stations[name], res.stations[name])


def test_a_failed_station_is_a_nan_row_or_an_error(station_pool):
    pool, c = station_pool, station_pool.chains_per_station
    inner = pool.pool
    keep = inner.iter.copy()
    try:
        it = inner.iter[3 * c + 1]                                  # a chain of DDD: its main phase begins 5 iterations
        early = (it >= 0) & (it < inner.iter_main - 5)              # before the end, so n = 2 < 4
        it[it < 0] -= inner.iter_main - 5
        it[early] -= inner.iter_main - 5
        res = pool.convergence(nlags=16, dev=0.5, exclude_outliers=False, strict=False)
        assert list(res.failed) == ['DDD'] and 'DDD' not in res.stations and 'window' in res.failed['DDD']
        for c_ in res.columns:
            assert np.isnan(res.rhat[c_][3]) and np.isnan(res.converged[c_][3]) and np.isnan(res.ess[c_][3])
            live = [not res.stations[n][c_]['constant'] for n in ('AAA', 'BBB', 'CCC', 'EEE')]   # (a fixed correlation)
            assert np.array_equal(np.isfinite(res.rhat[c_][[0, 1, 2, 4]]), live)
        assert np.isfinite(res.rhat['vpvs'][[0, 1, 2, 4]]).all() and set(res.converged['vpvs'][[0, 1, 2, 4]]) <= {0., 1.}
        assert tuple(res.window[3]) == (-1, -1)
        with pytest.raises(ValueError, match="station 'DDD'"):
            pool.convergence(nlags=16, dev=0.5, exclude_outliers=False)
        with pytest.raises(ValueError, match='window'):
            pool.station('DDD').convergence(nlags=16, dev=0.5, exclude_outliers=False)
    finally:
        inner.iter[:] = keep
