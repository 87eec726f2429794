"""GPU tier of the depth-to-depth covariance (bh_depthcov_sets, bayhunter_amd/covariance.py, ChainPool.depth_covariance,
StationPool.depth_covariance) against the numpy restatement (tests/depthcov_ref.py) within tests/depthcov_tolerances.py.

The host twin (tests/hostsim/depthcov_sim.cpp) accumulates one fma per row where the device issues one MFMA per four
rows; whether the two round alike is MEASURED here, not asserted: the number of cells that differ and their largest
relative difference go to profiles/r16_depthcov.jsonl (line 'twin')."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import depthcov_ref as ref  # noqa: E402
import depthcov_tolerances as tol  # noqa: E402
from test_depthcov import load_sim, sim_case  # noqa: E402

pytestmark = pytest.mark.gpu

PROFILE = os.path.join(ROOT, 'profiles', 'r16_depthcov.jsonl')
SHAPES = [(ndep, nextra) for ndep in (2, 16, 17, 33) for nextra in (0, 1, 3)]
# float32 rows with weights and float64 rows without over every shape; the other two pairings where K is odd
CASES = [(nd, ne, False, True) for nd, ne in SHAPES] + [(nd, ne, True, False) for nd, ne in SHAPES] + \
        [(17, 1, False, False), (17, 1, True, True), (33, 3, False, False), (33, 3, True, True)]


@pytest.fixture(scope='module')
def dsim():
    return load_sim()


@pytest.fixture(scope='module')
def twin_record():
    """Collects the device-against-twin comparison of every case; one 'twin' line replaces the profile's earlier one."""
    rec = dict(leg='twin', cases=0, cells=0, cells_differ=0, max_rel_diff=0., r1_cells=0, r1_cells_differ=0,
               r1_max_rel_diff=0.)
    yield rec
    from bayhunter_amd import _lib
    rec['src'] = _lib.loaded_hash()
    try:
        lines = []
        if os.path.exists(PROFILE):
            with open(PROFILE) as fh:
                lines = [l for l in fh.read().splitlines() if l.strip() and json.loads(l).get('leg') != 'twin']
        with open(PROFILE, 'w') as fh:
            fh.write('\n'.join([json.dumps(rec)] + lines) + '\n')
    except OSError as e:
        print('profile not written:', e)
    print('twin:', rec)


def depthcov(c, pad=0, expect=0, sets=None):
    """bh_depthcov_sets over a case's host arrays (uploaded; `pad` unused columns of 7.0 beyond the rows and the extras)
    -> (S, r1, total), or the error text.  sets = (set_start, center): other sets over the same rows."""
    import torch
    from bayhunter_amd import _lib
    lib = _lib.load()
    rows, w, extra = c['rows'], c['weights'], c['extra']
    R, W = rows.shape
    t = torch.full((R, W + pad), 7.0, dtype=torch.float64 if rows.dtype == np.float64 else torch.float32, device='cuda')
    t[:, :W] = torch.from_numpy(rows).cuda()
    dw = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.int32)).cuda()
    nextra = 0 if extra is None else extra.shape[1]
    de = None
    if nextra:
        de = torch.full((R, nextra + pad), 7.0, dtype=torch.float64, device='cuda')
        de[:, :nextra] = torch.from_numpy(extra).cuda()
    start, center = (c['set_start'], c['center']) if sets is None else sets
    start = np.ascontiguousarray(start, dtype=np.int64)
    center, dep = np.ascontiguousarray(center, dtype=np.float64), np.ascontiguousarray(c['dep'], dtype=np.float64)
    Z, K = start.size - 1, dep.size + nextra
    S, r1, total = np.full((Z, K, K), -7.), np.full((Z, K), -7.), np.full(Z, -1, dtype=np.int64)
    rc = lib.bh_depthcov_sets(t.data_ptr(), int(rows.dtype == np.float64), R, W + pad, W,
                              None if dw is None else dw.data_ptr(), None if de is None else de.data_ptr(), nextra + pad,
                              nextra, start.ctypes.data, Z, dep.ctypes.data, dep.size, center.ctypes.data, S.ctypes.data,
                              r1.ctypes.data, total.ctypes.data, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, lib.bh_last_error()
    return (S, r1, total) if rc == 0 else lib.bh_last_error().decode()


def sub_case(c, a, b, lead):
    """Rows a:b of a case behind `lead` other rows (the case's first ones)."""
    sl = lambda x: None if x is None else np.ascontiguousarray(np.concatenate((x[:lead], x[a:b])))
    return dict(rows=sl(c['rows']), weights=sl(c['weights']), extra=sl(c['extra']), dep=c['dep'])


def rel_diff(a, b):
    d = np.abs(a - b)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(d > 0, d / np.maximum(np.abs(a), np.abs(b)), 0.)
    return int((d > 0).sum()), float(r.max()) if r.size else 0.


@pytest.mark.parametrize('ndep,nextra,fp64,weighted', CASES)
def test_depthcov_sets_against_the_restatement(lib, dsim, twin_record, ndep, nextra, fp64, weighted):
    from bayhunter_amd import _lib
    B = _lib.DEPTHCOV_BLOCK_ROWS
    assert B == dsim.ds_block_rows()
    c = ref.case(B, ndep, nextra, fp64, weighted)
    assert c['counts'] == [1, 3, 0, 4, B, 5, B + 1, 2 * B + 5]
    want = ref.moments(c['rows'], c['weights'], c['extra'], c['set_start'], c['dep'], c['center'])
    S, r1, total = depthcov(c, pad=3)
    # 1. the bound on every cell of S and r1, total exact; an empty set and a set of weight 0: zeros
    worst = tol.check_moments(S, r1, total, want, 'ndep %d nextra %d' % (ndep, nextra))
    print('ndep %d nextra %d fp64 %d weighted %d: worst |difference| / bound %.3g' % (ndep, nextra, fp64, weighted, worst))
    assert total[2] == 0 and total[5] == 0 and not np.any(S[[2, 5]]) and not np.any(r1[[2, 5]])
    # 2. exactly symmetric
    assert np.array_equal(S, np.swapaxes(S, 1, 2))
    # 3. two runs (and no stride in the result)
    S2, r12, total2 = depthcov(c)
    assert S.tobytes() == S2.tobytes() and r1.tobytes() == r12.tobytes() and np.array_equal(total, total2)
    # 4. every set alone with nsets = 1 ... and at another offset in rows, behind a set of three other rows
    st = c['set_start']
    for z in range(len(st) - 1):
        a, b = int(st[z]), int(st[z + 1])
        if a == b:
            continue
        Sz, rz, tz = depthcov(sub_case(c, a, b, 0), sets=([0, b - a], c['center'][z:z + 1]))
        assert Sz[0].tobytes() == S[z].tobytes() and rz[0].tobytes() == r1[z].tobytes() and tz[0] == total[z], z
        Sz, rz, tz = depthcov(sub_case(c, a, b, 3), sets=([0, 3, 3 + b - a], c['center'][[0, z]]))
        assert Sz[1].tobytes() == S[z].tobytes() and rz[1].tobytes() == r1[z].tobytes() and tz[1] == total[z], z
    # 8. the twin, measured and not asserted
    St, rt, tt = sim_case(dsim, c)
    assert np.array_equal(tt, total)
    n, r = rel_diff(S, St)
    n1, rr = rel_diff(r1, rt)
    twin_record['cases'] += 1
    twin_record['cells'] += int(S.size)
    twin_record['cells_differ'] += n
    twin_record['max_rel_diff'] = max(twin_record['max_rel_diff'], r)
    twin_record['r1_cells'] += int(r1.size)
    twin_record['r1_cells_differ'] += n1
    twin_record['r1_max_rel_diff'] = max(twin_record['r1_max_rel_diff'], rr)


def test_more_blocks_than_one_launch_takes(lib):
    """One set of 1 025 blocks and three rows: the slab holds 1 024 blocks, the fold goes on in a second run."""
    from bayhunter_amd import _lib
    rng = np.random.default_rng(77)
    R = 1025 * _lib.DEPTHCOV_BLOCK_ROWS + 3
    rows = np.full((R, ref.WIDTH), np.nan, dtype=np.float32)
    rows[:, :2] = rng.uniform(2., 5., (R, 2))
    rows[:, 2:4] = np.sort(rng.uniform(0., 60., (R, 2)), axis=1)
    c = dict(rows=rows, weights=None, extra=None, set_start=np.asarray([0, 5, R]), dep=np.asarray([20., 45.]))
    c['center'] = np.asarray([[3.4, 3.6], [3.5, 3.5]])
    want = ref.moments(rows, None, None, c['set_start'], c['dep'], c['center'])
    S, r1, total = depthcov(c)
    tol.check_moments(S, r1, total, want, 'two runs')
    assert total.tolist() == [5, R - 5] and np.array_equal(S, np.swapaxes(S, 1, 2))
    S2, r12, _ = depthcov(c)
    assert S.tobytes() == S2.tobytes() and r1.tobytes() == r12.tobytes()


def test_refusals_on_the_device(lib):
    from bayhunter_amd import _lib
    c = ref.case(_lib.DEPTHCOV_BLOCK_ROWS, 17, 1, False, True)
    bad = dict(c, weights=c['weights'].copy())
    bad['weights'][-1] = -1
    assert 'negative weight' in depthcov(bad, expect=_lib.BH_ERR_ARG)
    assert 'ascending' in depthcov(dict(c, dep=c['dep'][::-1]), expect=_lib.BH_ERR_ARG)
    assert 'ndep' in depthcov(dict(c, dep=c['dep'][:0], center=c['center'][:, 17:]), expect=_lib.BH_ERR_ARG)
    wide = dict(c, dep=np.arange(256.), center=np.zeros((8, 257)))
    assert 'above 256' in depthcov(wide, expect=_lib.BH_ERR_ARG)
    assert 'set_start' in depthcov(c, sets=([0, 7, 5, c['rows'].shape[0]], c['center'][:3]), expect=_lib.BH_ERR_ARG)
    assert 'set_start' in depthcov(c, sets=([0, 7, c['rows'].shape[0] - 1], c['center'][:2]), expect=_lib.BH_ERR_ARG)
    S, _, total = depthcov(c)                                          # and the library goes on
    assert total[4] > 0 and np.array_equal(S, np.swapaxes(S, 1, 2))


def same_result(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype.kind == 'f':
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert np.array_equal(a[k], b[k]), k


def test_summarize_sets_equals_summarize_per_set(lib):
    from bayhunter_amd import _lib, covariance as cv
    c = ref.case(_lib.DEPTHCOV_BLOCK_ROWS, 17, 1, False, True)
    kw = dict(dep_int=c['dep'], extra_names=('vpvs',))
    res = cv.summarize_sets(c['rows'], c['set_start'], c['weights'], extra=c['extra'], strict=False, **kw)
    assert sorted(res.failed) == [2, 5] and res[2] is None and res[5] is None
    with pytest.raises(ValueError, match='set 2'):
        cv.summarize_sets(c['rows'], c['set_start'], c['weights'], extra=c['extra'], **kw)
    runs = cv.summarize_sets(c['rows'], c['set_start'], c['weights'], extra=c['extra'], strict=False, budget_bytes=1, **kw)
    st = c['set_start']
    for z in range(len(st) - 1):
        a, b = int(st[z]), int(st[z + 1])
        if z in res.failed:
            if b > a:
                with pytest.raises(ValueError, match='empty selection'):
                    cv.summarize(c['rows'][a:b], c['weights'][a:b], extra=c['extra'][a:b], **kw)
            continue
        one = cv.summarize(c['rows'][a:b], c['weights'][a:b], extra=c['extra'][a:b], **kw)
        same_result(res[z], one)
        same_result(runs[z], one)                                      # one set per call: no result depends on the budget
        assert one['names'] == ['vs@%g' % d for d in c['dep']] + ['vpvs'] and one['cov'].shape == (18, 18)
        assert one['nmodels'] == int(c['weights'][a:b][~np.isnan(c['rows'][a:b, 0])].sum())
        flat = one['std'] == 0
        assert np.all(np.isnan(one['corr'][flat])) and np.all(np.isnan(one['corr'][:, flat]))
        assert np.all(np.diagonal(one['corr'])[~flat] == 1.) and np.array_equal(one['cov'], one['cov'].T)
    assert np.all(res[0]['std'] == 0) and np.all(np.isnan(res[0]['corr']))        # one row: no variance anywhere
    # against the restatement, with the centre the package took
    want = ref.moments(c['rows'], c['weights'], c['extra'], st, c['dep'],
                       np.stack([np.zeros(18) if r is None else r['mean'] for r in res]))
    for z in (3, 4, 6, 7):
        wcov, _ = ref.cov_corr(want['S'][z], want['r1'][z], want['total'][z])
        assert np.all(np.abs(res[z]['cov'] - wcov) <= tol.cov_bound(want, z)), z


# ---- pools --------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def chain_pool(lib):
    from bayhunter_amd.chains import GpuEvaluator
    from chain_scenario import CASES, make_pool
    case = dict(CASES['tutorial'], burnin=200, main=300)
    return make_pool(None, os.path.join(GOLDEN, 'tutorial_observed'), case, seeds=list(range(41, 47)),
                     evaluator=GpuEvaluator).run()


@pytest.fixture(scope='module')
def station_pool(lib):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=150, iter_main=300)
    names = ['AAA', 'BBB', 'CCC']
    stations = make_stations(os.path.join(GOLDEN, 'tutorial_observed'), 3, refs=case.get('refs', ('rdispph', 'prf')), yerr=True)
    with StationPool(dict(zip(names, stations)), ip, case['priors'], chains_per_station=2, random_seeds=[51, 52, 53],
                     nmodels=451) as pool:
        pool.run()
    return pool


def test_chain_pool_depth_covariance_equals_the_restatement(chain_pool):
    from bayhunter_amd.selection import pool_rows
    pool, dep = chain_pool, np.linspace(0., 100., 201)
    got = pool.depth_covariance(dev=0.5)                               # the default grid: 201 depths and vpvs, 91 tile pairs
    ci, ri, w = pool_rows(pool, 'weighted', 0.5, True)
    assert got['names'] == ['vs@%g' % d for d in dep] + ['vpvs'] and got['cov'].shape == (202, 202)
    assert got['nmodels'] == w.sum() and np.array_equal(got['chains'], np.unique(ci) + pool.first)
    extra = pool.vpvs[ci, ri].astype(np.float64)[:, None]
    want = ref.moments(pool.models[ci, ri], w, extra, [0, ci.size], dep, got['mean'][None, :])
    assert want['total'][0] == got['nmodels']
    # the scan's mean is the weighted mean to the rounding of its own sum: r1 / W, what the centre is off, is that small
    X, _ = ref.columns(pool.models[ci, ri], dep, extra)
    exact = (w[:, None].astype(np.longdouble) * X).sum(axis=0) / np.longdouble(w.sum())
    assert np.all(np.abs(got['mean'] - exact) <= tol.gamma(ci.size + 2) * np.abs(X).max(axis=0))
    wcov, wcorr = ref.cov_corr(want['S'][0], want['r1'][0], want['total'][0])
    bound = tol.cov_bound(want, 0)
    flat = got['std'] == 0
    live = np.ix_(~flat, ~flat)
    assert np.all(np.abs(got['cov'] - wcov)[live] <= bound[live])
    assert np.all(np.abs(wcov[flat]) <= bound[flat]) and not np.any(got['cov'][flat]) and not np.any(got['cov'][:, flat])
    assert np.array_equal(got['cov'], got['cov'].T) and np.array_equal(got['std'], np.sqrt(np.diagonal(got['cov'])))
    assert np.all(np.isnan(got['corr'][flat])) and np.all(np.isnan(got['corr'][:, flat]))
    assert np.all(np.diagonal(got['corr'])[~flat] == 1.) and np.all(np.abs(got['corr'][live]) <= 1 + 1e-12)
    assert (~flat).sum() > 100                                         # a tutorial pool moves at most depths
    # no extras, a grid of one's own, the saved selection
    small = pool.depth_covariance(dep_int=[0., 10., 35., 70.], extras=(), selection='saved', dev=0.5)
    assert small['names'] == ['vs@0', 'vs@10', 'vs@35', 'vs@70'] and small['cov'].shape == (4, 4)
    with pytest.raises(ValueError, match='extras'):
        pool.depth_covariance(extras=('moho',))


def test_station_pool_depth_covariance_equals_every_station_view(station_pool):
    pool = station_pool
    kw = dict(extras=('vpvs', 'sigma:prf'), dev=0.5)
    res = pool.depth_covariance(**kw)
    assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and sorted(res.stations) == res.names
    assert res.columns[0] == 'vs@0' and res.columns[-2:] == ['vpvs', 'sigma:prf'] and len(res.columns) == 203
    assert res.cov.shape == res.corr.shape == (3, 203, 203) and res.mean.shape == res.std.shape == (3, 203)
    runs = pool.depth_covariance(max_rows=1, budget_bytes=1, **kw)     # a station per run and per call
    for s, name in enumerate(res.names):
        one = pool.station(name).depth_covariance(**kw)
        same_result(res.stations[name], one)
        same_result(runs.stations[name], one)
        assert one['names'] == res.columns and res.nmodels[s] == one['nmodels']
        for k in ('cov', 'corr', 'mean', 'std'):
            assert getattr(res, k)[s].tobytes() == one[k].tobytes(), (name, k)
