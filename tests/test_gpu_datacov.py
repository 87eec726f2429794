"""GPU tier of the cross-covariance of Vs(z) and the modelled data (bh_datacov_sets, bayhunter_amd/datacov.py,
ChainPool.data_covariance, StationPool.data_covariance) against the numpy restatement (tests/datacov_ref.py) within
tests/datacov_tolerances.py.

The host twin (tests/hostsim/datacov_sim.cpp) accumulates one fma per row where the device issues one MFMA per four
rows; whether the two round alike is MEASURED here, not asserted: the number of cells that differ and their largest
relative difference go to profiles/datacov.jsonl (line 'twin')."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import datacov_ref as ref  # noqa: E402
import datacov_tolerances as tol  # noqa: E402
import depthcov_ref as dref  # noqa: E402
import depthcov_tolerances as dtol  # noqa: E402
from test_datacov import NAMES, load_sim, outputs, same_bits, sim, sub_case, want_of  # noqa: E402

pytestmark = pytest.mark.gpu

PROFILE = os.path.join(ROOT, 'profiles', 'datacov.jsonl')
SHAPES = [(2, 0), (17, 1), (33, 3)]
WIDE = 257                       # one column more than a group of data columns holds at these K (asserted below)
WIDTHS = [1, 16, 17, 40, WIDE]
# float32 rows with weights and float64 rows without over every shape and width; the other two pairings at the widest
CASES = [(nd, ne, S, False, True) for nd, ne in SHAPES for S in WIDTHS] + \
        [(nd, ne, S, True, False) for nd, ne in SHAPES for S in WIDTHS] + \
        [(17, 1, WIDE, False, False), (33, 3, WIDE, True, True)]


@pytest.fixture(scope='module')
def dsim():
    return load_sim()


@pytest.fixture(scope='module')
def twin_record():
    """Collects the device-against-twin comparison of every case; one 'twin' line replaces the profile's earlier one."""
    rec = dict(leg='twin', cases=0)
    for k in NAMES[:5]:
        rec.update({k + '_cells': 0, k + '_cells_differ': 0, k + '_max_rel_diff': 0.})
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


def datacov(c, pad=0, expect=0, cols=None):
    """bh_datacov_sets over a case's host arrays (uploaded; `pad` unused columns of 7.0 beyond the rows, the extras, the
    data and the flags) -> dict(C, r1x, r1y, qx, qy, total, excluded), or the error text.  cols = (col0, S): those columns
    of the case's Y as the data columns."""
    import torch
    from bayhunter_amd import _lib
    lib = _lib.load()
    rows, w, extra, Y, err = c['rows'], c['weights'], c['extra'], c['Y'], c['err']
    R, W = rows.shape

    def up(a, dtype):
        t = torch.full((R, a.shape[1] + pad), 7, dtype=dtype, device='cuda')
        t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t
    t = up(rows, torch.float64 if rows.dtype == np.float64 else torch.float32)
    dw = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.int32)).cuda()
    nextra = 0 if extra is None else extra.shape[1]
    de = up(extra, torch.float64) if nextra else None
    dY, derr = up(Y, torch.float64), up(err, torch.int32)
    col0, S = (0, Y.shape[1]) if cols is None else cols
    start = np.ascontiguousarray(c['set_start'], dtype=np.int64)
    dep, cx, cy = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ('dep', 'cx', 'cy'))
    Z, K = start.size - 1, dep.size + nextra
    out, ptrs = outputs(Z, K, S)
    rc = lib.bh_datacov_sets(t.data_ptr(), int(rows.dtype == np.float64), R, W + pad, W,
                             None if dw is None else dw.data_ptr(), None if de is None else de.data_ptr(), nextra + pad,
                             nextra, dY.data_ptr(), Y.shape[1] + pad, col0, S, derr.data_ptr(), err.shape[1] + pad,
                             err.shape[1], start.ctypes.data, Z, dep.ctypes.data, dep.size, cx.ctypes.data, cy.ctypes.data,
                             *(ptrs + [torch.cuda.current_stream().cuda_stream]))
    assert rc == expect, lib.bh_last_error()
    return out if rc == 0 else lib.bh_last_error().decode()


def rel_diff(a, b):
    d = np.abs(a - b)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(d > 0, d / np.maximum(np.abs(a), np.abs(b)), 0.)
    return int((d > 0).sum()), float(r.max()) if r.size else 0.


@pytest.mark.parametrize('ndep,nextra,S,fp64,weighted', CASES)
def test_datacov_sets_against_the_restatement(lib, dsim, twin_record, ndep, nextra, S, fp64, weighted):
    from bayhunter_amd import _lib
    B = _lib.DEPTHCOV_BLOCK_ROWS
    assert B == dsim.dcs_block_rows() and dsim.dcs_group_cols(ndep + nextra) == WIDE - 1
    c = ref.case(B, ndep, nextra, S, fp64, weighted)
    assert c['counts'] == [1, 3, 0, 4, B, 5, B + 1, 2 * B + 5]
    want = want_of(c)
    got = datacov(c, pad=3)
    # 1. the bound on every cell of every moment, total and excluded exact; an empty set and a set without a row that
    #    counts: zeros
    worst = tol.check_moments(got, want, 'ndep %d nextra %d S %d' % (ndep, nextra, S))
    print('ndep %d nextra %d S %d fp64 %d weighted %d: worst |difference| / bound %.3g' % (ndep, nextra, S, fp64, weighted,
                                                                                           worst))
    assert got['total'][2] == 0 and got['total'][5] == 0 and got['excluded'][5] == (0 if weighted else 5)
    assert got['excluded'][7] > 0                                      # flagged rows and rows with a NaN in the last group
    for k in NAMES[:5]:
        assert not np.any(got[k][[2, 5]]), k
    # 2. two runs (and no stride in the result)
    same_bits(got, datacov(c))
    # 3. every set alone with nsets = 1 ... and at another offset in rows, behind a set of three other rows
    st = c['set_start']
    for z in range(len(st) - 1):
        a, b = int(st[z]), int(st[z + 1])
        if a == b:
            continue
        same_bits(datacov(sub_case(c, a, b, 0, z)), got, slice(0, 1), slice(z, z + 1), z)
        same_bits(datacov(sub_case(c, a, b, 3, z)), got, slice(1, 2), slice(z, z + 1), z)
    # 4. the twin, measured and not asserted
    tw = sim(dsim, c)
    assert np.array_equal(tw['total'], got['total']) and np.array_equal(tw['excluded'], got['excluded'])
    twin_record['cases'] += 1
    for k in NAMES[:5]:
        n, r = rel_diff(got[k], tw[k])
        twin_record[k + '_cells'] += int(got[k].size)
        twin_record[k + '_cells_differ'] += n
        twin_record[k + '_max_rel_diff'] = max(twin_record[k + '_max_rel_diff'], r)


@pytest.mark.parametrize('ndep,nextra', SHAPES)
def test_a_column_subset_keeps_its_bits(lib, ndep, nextra):
    """Without NaN rows the rows that count do not depend on the data columns: columns on both sides of the boundary
    between two groups give the same bits when they are the only data columns -- of the same Y, and of a Y that holds
    nothing else."""
    from bayhunter_amd import _lib
    c = ref.case(_lib.DEPTHCOV_BLOCK_ROWS, ndep, nextra, WIDE, False, True, nans=False)
    got = datacov(c)
    a, n = WIDE - 9, 9
    sub = datacov(dict(c, cy=c['cy'][:, a:]), cols=(a, n), pad=2)
    narrow = datacov(dict(c, Y=np.ascontiguousarray(c['Y'][:, a:]), cy=c['cy'][:, a:]))
    for part in (sub, narrow):
        assert part['C'].tobytes() == np.ascontiguousarray(got['C'][:, :, a:]).tobytes()
        for k in ('r1y', 'qy'):
            assert part[k].tobytes() == np.ascontiguousarray(got[k][:, a:]).tobytes(), k
        for k in ('r1x', 'qx', 'total', 'excluded'):
            assert part[k].tobytes() == got[k].tobytes(), k


def test_more_blocks_than_one_launch_takes(lib):
    """One set of 1 025 blocks and three rows: the slab holds 1 024 blocks, the fold goes on in a second run."""
    from bayhunter_amd import _lib
    rng = np.random.default_rng(77)
    R = 1025 * _lib.DEPTHCOV_BLOCK_ROWS + 3
    rows = np.full((R, dref.WIDTH), np.nan, dtype=np.float32)
    rows[:, :2] = rng.uniform(2., 5., (R, 2))
    rows[:, 2:4] = np.sort(rng.uniform(0., 60., (R, 2)), axis=1)
    Y = rng.uniform(-1., 1., (R, 3)) + rows[:, :1]
    err = np.zeros((R, 1), dtype=np.int32)
    err[rng.integers(0, R, 1000)] = 2
    c = dict(rows=rows, weights=None, extra=None, Y=Y, err=err, set_start=np.asarray([0, 5, R]),
             dep=np.asarray([20., 45.]), cx=np.asarray([[3.4, 3.6], [3.5, 3.5]]), cy=np.asarray([[3.5] * 3, [3.4, 3.5, 3.6]]))
    want = want_of(c)
    got = datacov(c)
    tol.check_moments(got, want, 'two runs')
    assert got['total'].sum() + got['excluded'].sum() == R and got['excluded'][1] > 900
    same_bits(got, datacov(c))


def test_refusals_on_the_device(lib):
    from bayhunter_amd import _lib
    c = ref.case(_lib.DEPTHCOV_BLOCK_ROWS, 17, 1, 17, False, True)
    E = _lib.BH_ERR_ARG
    bad = dict(c, weights=c['weights'].copy())
    bad['weights'][-1] = -1
    assert 'negative weight' in datacov(bad, expect=E)
    assert 'ascending' in datacov(dict(c, dep=c['dep'][::-1]), expect=E)
    assert 'ndep' in datacov(dict(c, dep=c['dep'][:0], cx=c['cx'][:, 17:]), expect=E)
    assert 'above 256' in datacov(dict(c, dep=np.arange(256.), cx=np.zeros((8, 257))), expect=E)
    assert 'data columns' in datacov(dict(c, cy=np.zeros((8, 0))), cols=(0, 0), expect=E)
    assert 'y_stride' in datacov(dict(c, cy=np.zeros((8, 5))), cols=(13, 5), expect=E)
    n = c['rows'].shape[0]
    assert 'set_start' in datacov(dict(c, set_start=[0, 7, 5, n], cx=c['cx'][:3], cy=c['cy'][:3]), expect=E)
    assert 'set_start' in datacov(dict(c, set_start=[0, 7, n - 1], cx=c['cx'][:2], cy=c['cy'][:2]), expect=E)
    got = datacov(c)                                                   # and the library goes on
    assert got['total'][4] > 0
    tol.check_moments(got, want_of(c), 'after the refusals')


# ---- the Python layer -------------------------------------------------------------------------------------------

def same_result(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype.kind == 'f':
            assert a[k].tobytes() == b[k].tobytes(), k
        elif isinstance(a[k], dict):
            assert sorted(a[k]) == sorted(b[k]) and all(np.array_equal(a[k][r], b[k][r]) for r in a[k]), k
        else:
            assert np.array_equal(a[k], b[k]), k


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


def test_chain_pool_data_covariance_equals_the_restatement(chain_pool):
    import torch
    from bayhunter_amd import covariance as cv, datacov as dc, datafits as df, posterior as post
    from bayhunter_amd.selection import pool_rows
    pool, dep = chain_pool, np.linspace(0., 100., 201)
    got = pool.data_covariance(dev=0.5)                                # the default grid: 201 depths and vpvs
    fits = pool.datafits(dev=0.5)
    ci, ri, w = pool_rows(pool, 'weighted', 0.5, True)
    S = sum(t['mean'].size for t in fits['targets'])
    assert got['names'] == ['vs@%g' % d for d in dep] + ['vpvs'] and got['cov'].shape == got['corr'].shape == (202, S)
    assert np.array_equal(got['chains'], np.unique(ci) + pool.first) and np.array_equal(got['dep'], dep)
    # the data side is datafits()': the same rows, the same means bit for bit
    assert got['nmodels'] == fits['nmodels'] and got['nexcluded'] == fits['nexcluded']
    assert got['nmodels'] + got['nexcluded'] == w.sum()
    for t, tg in zip(fits['targets'], pool.targets.targets):
        sl = got['targets'][tg.ref]
        assert got['mean_y'][sl].tobytes() == t['mean'].tobytes() and np.array_equal(got['x'][tg.ref], tg.obsdata.x)
    # the restatement on the pool's rows and the modelled data the forward pass returns, with the centres the package
    # takes: the posterior scan's mean of Vs, the column scan's mean of vpvs, the data scan's mean of the data
    models, vpvs = pool.models[ci, ri], pool.vpvs[ci, ri].astype(np.float64)
    _, Y, err, _ = df.forward_matrix(pool.targets, models, vpvs, pool.priors.get('mantle'))
    Yh, errh = Y[:, :S].cpu().numpy(), err.cpu().numpy()
    stream = torch.cuda.current_stream().cuda_stream
    dw = torch.from_numpy(w.astype(np.int32)).cuda()
    with post.Sets(torch.from_numpy(models).cuda(), dw, None, np.asarray([0, ci.size]), dep, None, stream) as g:
        cx = g.scan()['mean'][0]
    with dc.ColumnScan(torch.from_numpy(vpvs[:, None].copy()).cuda(), 1, dw, None, [0, ci.size], stream) as f:
        cx = np.concatenate((cx, f.scan()['mean'][0]))
    want = ref.moments(models, w, vpvs[:, None], Yh, errh, [0, ci.size], dep, cx[None, :], got['mean_y'][None, :])
    assert want['total'][0] == got['nmodels'] and want['excluded'][0] == got['nexcluded']
    wcov, bound = ref.cov(want, 0), tol.cov_bound(want, 0)
    flat = np.isnan(got['corr'])
    print('cov: worst |difference| / bound %.3g over %d live cells' % (float((np.abs(got['cov'] - wcov)[~flat] /
                                                                        bound[~flat]).max()), (~flat).sum()))
    assert np.all(np.abs(got['cov'] - wcov)[~flat] <= bound[~flat])
    assert not np.any(got['cov'][flat]) and (~flat).sum() > 100 * S // 2
    assert np.all(np.abs(got['corr'][~flat]) <= 1 + 1e-12)
    W = np.longdouble(want['total'][0])
    assert np.all(np.abs(got['mean_x'] - (cx + want['r1x'][0] / W)) <=
                  tol.moment_bounds(want, 0)['r1x'] / W + 2 * tol.U * np.abs(cx))
    # std_x against depth_covariance()'s over the rows that count
    _, ok = ref.counts(models, w, Yh, errh, dep)
    depth = cv.summarize(models, np.where(ok, w, 0).astype(np.int32), dep, vpvs[:, None], ('vpvs',))
    dwant = dref.moments(models, np.where(ok, w, 0), vpvs[:, None], [0, ci.size], dep, depth['mean'][None, :])
    vx, _ = ref.variances(want, 0)
    dvar = np.diagonal(dref.cov_corr(dwant['S'][0], dwant['r1'][0], dwant['total'][0])[0])
    b = tol.std_bound(vx, tol.var_bounds(want, 0, recentred=True)[0]) + \
        tol.std_bound(dvar, np.diagonal(dtol.cov_bound(dwant, 0, recentred=True)))
    live = (got['std_x'] > 0) & (depth['std'] > 0)
    assert live.sum() > 100 and np.all(np.abs(got['std_x'] - depth['std'])[live] <= b[live])
    # no extras, a grid of one's own, the saved selection
    small = pool.data_covariance(dep_int=[0., 10., 35., 70.], extras=(), selection='saved', dev=0.5)
    assert small['names'] == ['vs@0', 'vs@10', 'vs@35', 'vs@70'] and small['cov'].shape == (4, S)
    with pytest.raises(ValueError, match='extras'):
        pool.data_covariance(extras=('moho',))


def test_station_pool_data_covariance_equals_every_station_view(station_pool):
    pool = station_pool
    kw = dict(extras=('vpvs', 'sigma:prf'), dev=0.5)
    res = pool.data_covariance(**kw)
    assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and sorted(res.stations) == res.names
    assert res.columns[0] == 'vs@0' and res.columns[-2:] == ['vpvs', 'sigma:prf'] and len(res.columns) == 203
    S = res.mean_y.shape[1]
    assert res.cov.shape == res.corr.shape == (3, 203, S) and res.mean_x.shape == res.std_x.shape == (3, 203)
    runs = pool.data_covariance(max_rows=1, **kw)                      # a station per run
    for s, name in enumerate(res.names):
        one = pool.station(name).data_covariance(**kw)
        same_result(res.stations[name], one)
        same_result(runs.stations[name], one)
        assert one['names'] == res.columns and res.nmodels[s] == one['nmodels'] and res.nexcluded[s] == one['nexcluded']
        for k in ('cov', 'corr', 'mean_x', 'std_x', 'mean_y', 'std_y'):
            assert getattr(res, k)[s].tobytes() == one[k].tobytes(), (name, k)
    # one station made to fail: BBB loses its main-phase rows
    inner = pool.pool
    keep = inner.iter[2:4].copy()
    try:
        inner.iter[2:4] = -1
        part = pool.data_covariance(strict=False, **kw)
        with pytest.raises(ValueError, match='BBB'):
            pool.data_covariance(**kw)
    finally:
        inner.iter[2:4] = keep
    assert sorted(part.failed) == ['BBB'] and 'empty selection' in part.failed['BBB'] and sorted(part.stations) == ['AAA', 'CCC']
    assert np.all(np.isnan(part.cov[1])) and part.nmodels[1] == 0
    for name in ('AAA', 'CCC'):
        same_result(part.stations[name], res.stations[name])


# ---- physics ------------------------------------------------------------------------------------------------

def test_phase_velocity_follows_the_shear_velocity_of_the_layer_that_moves(lib):
    """64 models of two layers over a half-space that differ in the Vs of the second layer alone: every Rayleigh phase
    velocity rises with it (the derivative of phase velocity with respect to shear velocity is positive), and Vs at a
    depth outside that layer is one value: no correlation to speak of."""
    from bayhunter_amd import datacov as dc, targets as T
    per = np.linspace(4., 40., 13)
    joint = T.JointTarget([T.RayleighDispersionPhase(per, np.full(per.size, 3.5))])
    models = np.full((64, 12), np.nan)
    models[:, :3] = (3.0, 3.5, 4.5)
    models[:, 1] = np.linspace(3.3, 3.9, 64)
    models[:, 3:6] = (2., 10., 40.)                                   # nuclei: interfaces at 6 and 25 km
    dep = np.asarray([1., 5., 7., 15., 24., 26., 60.])
    inside = np.asarray([False, False, True, True, True, False, False])
    for m in (models, models.astype(np.float32)):
        res = dc.summarize(joint, m, 1.73, dep_int=dep)
        assert res['nmodels'] == 64 and res['nexcluded'] == 0 and res['cov'].shape == (7, per.size)
        assert list(res['targets']) == ['rdispph'] and res['targets']['rdispph'] == slice(0, per.size)
        assert np.all(res['corr'][inside] > 0) and np.all(res['cov'][inside] > 0)
        assert np.all(np.isnan(res['corr'][~inside])) and not np.any(res['cov'][~inside]) and not np.any(res['std_x'][~inside])
        assert np.all(res['std_y'] > 0) and np.allclose(res['mean_x'][inside], models[:, 1].mean(), rtol=0, atol=1e-6)
