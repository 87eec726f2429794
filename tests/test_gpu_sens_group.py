"""Group-velocity sensitivity kernels on the device.

* bh_sens_group_batch returns, bit for bit, the host twin built with the device's math (tests/hostsim/sens_group_sim.cpp)
  -- which tests/test_sens_group.py holds to the longdouble reference -- at the lane layouts where the indexing can go
  wrong (LAYOUTS): 8, exactly 64 and 68 slots per (model, period), 1 and 5 periods, blocks that span more than two
  models and a partial last block, ragged models with garbage behind their last layer and in the strides' padding, rows
  without a value between live ones.  At most 64 models.
* K_phase and c are bh_sens_batch's bits; bh_group_sensitivity and the plugin are the batch of one;
  ForwardEngine.group_sensitivity on a group target (through its companion phase engine) is the same call on an equal
  phase target.
* ChainPool.group_sensitivity() on a pool inverted with rdispgr + prf lies within the derived bounds
  (tests/sens_sets_tolerances.py) of the numpy restatement group_batch + vs_total + to_depth, whatever max_rows is;
  StationPool.group_sensitivity() is, station by station, bit for bit what the station's view returns.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import sens_group_cases as gc
import sensitivity_cases as sc
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import sens_sets_tolerances as sets_tol  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, 'tutorial_observed')
NAMES = list(sc.MODELS)
OUT = ('K', 'U', 'dU_dT', 'c', 'K_phase')


@pytest.fixture(scope='module')
def twin():
    return gc.load_sim()


def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(device='cuda', dtype=dtype)


def _group_batch(lib, M, nlay, per, wave, c, c_err, Lmax, k_phase=True):
    import torch
    from bayhunter_amd import _lib
    B, nper = nlay.size, per.size
    d = [_dev(M[i], torch.float64) for i in range(4)]
    dn, dper, dc, de = _dev(nlay, torch.int32), _dev(per, torch.float64), _dev(c, torch.float64), _dev(c_err, torch.int32)
    K, Kp = (torch.full((B, nper, 4, Lmax), -777.0, dtype=torch.float64, device='cuda') for _ in range(2))
    U, dU, co = (torch.full((B, nper), -777.0, dtype=torch.float64, device='cuda') for _ in range(3))
    need = lib.bh_sens_group_workspace_bytes(B, nper)
    ws = torch.empty(need // 8, dtype=torch.float64, device='cuda')
    _lib.check(lib.bh_sens_group_batch(B, Lmax, M.shape[2], dn.data_ptr(), *[x.data_ptr() for x in d], sc.WAVES[wave], nper,
                                       dper.data_ptr(), 0, dc.data_ptr(), c.shape[1], de.data_ptr(), c_err.shape[1],
                                       K.data_ptr(), U.data_ptr(), dU.data_ptr(), co.data_ptr(),
                                       Kp.data_ptr() if k_phase else None, ws.data_ptr(), need, None))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (K, U, dU, co, Kp))


def _phase_batch(lib, M, nlay, per, wave, c, c_err, Lmax):
    import torch
    from bayhunter_amd import _lib
    B, nper = nlay.size, per.size
    d = [_dev(M[i], torch.float64) for i in range(4)]
    dn, dper, dc, de = _dev(nlay, torch.int32), _dev(per, torch.float64), _dev(c, torch.float64), _dev(c_err, torch.int32)
    K = torch.empty((B, nper, 4, Lmax), dtype=torch.float64, device='cuda')
    co, dT = (torch.empty((B, nper), dtype=torch.float64, device='cuda') for _ in range(2))
    need = lib.bh_sens_workspace_bytes(B, nper)
    ws = torch.empty(need // 8, dtype=torch.float64, device='cuda')
    _lib.check(lib.bh_sens_batch(B, Lmax, M.shape[2], dn.data_ptr(), *[x.data_ptr() for x in d], sc.WAVES[wave], nper,
                                 dper.data_ptr(), 0, dc.data_ptr(), c.shape[1], de.data_ptr(), c_err.shape[1], K.data_ptr(),
                                 co.data_ptr(), dT.data_ptr(), ws.data_ptr(), need, None))
    torch.cuda.synchronize()
    return K.cpu().numpy(), co.cpu().numpy(), dT.cpu().numpy()


# name -> (Lmax, nper, B).  256 lanes per block, 64 per wave, 4 Lmax slots per (model, period):
LAYOUTS = {
    '2x1x41': (2, 1, 41),        # 8 slots: eight (model, period) pairs per wave, 32 models per block
    '2x5x41': (2, 5, 41),        # 40 lanes per model: a block spans 7 or 8 models, pairs straddle waves
    '16x1x9': (16, 1, 9),        # 64 slots: exactly one wave per (model, period), four models per block
    '16x5x7': (16, 5, 7),        # 320 lanes per model: a block starts inside a model
    '17x1x9': (17, 1, 9),        # 68 slots: just over one wave; a block spans 4 or 5 models
    '17x5x7': (17, 5, 7),
}
PAD = 3
_DATA = {}


def _check_layout(name):
    """What a layout is there for, as preconditions of the test that runs it."""
    Lmax, nper, B = LAYOUTS[name]
    per_model = nper * 4 * Lmax
    total = B * per_model
    assert B <= 64 and total % 256 != 0 and total > 256, name                       # several blocks, the last one partial
    spans = [min((g0 + 255) // per_model, B - 1) - g0 // per_model + 1 for g0 in range(0, total, 256)]
    assert max(spans) <= 255 // per_model + 2, name                                 # what the LDS image reserves
    if nper == 1:
        assert max(spans) > 2, name                                                # a workgroup spans more than two models
    assert 4 * Lmax in (8, 64, 68), name


def _layout(twin, name, wave):
    """The models, phase velocities and the twin's rows of one layout, built once: ragged models cut from
    sensitivity_cases.MODELS by deepen(), garbage behind each row's last layer and in the strides' padding, and the
    rows without a value (sensitivity_cases.NO_VALUE) mixed in."""
    if (name, wave) in _DATA:
        return _DATA[(name, wave)]
    Lmax, nper, B = LAYOUTS[name]
    rng = np.random.RandomState(2000 + Lmax + B)
    M = rng.choice([np.nan, 1e30, -1.0, 0.0, 7.7], size=(4, B, Lmax + PAD))
    nlay = np.zeros(B, dtype=np.int32)
    fit = [n for n in NAMES if len(sc.MODELS[n][0]) <= Lmax]
    for b in range(B):
        base = sc.MODELS[fit[b % len(fit)]]
        lo = len(base[0])
        n = Lmax if b == 1 else lo + (5 * b + 3 * (b // len(fit))) % (Lmax - lo + 1)
        s = 1.0 + 0.003 * (b // len(fit))
        h, vp, vs, rho = sc.deepen(base, n) if n > lo else base
        nlay[b] = n
        for i, x in enumerate((h, vp * s, vs * s, rho)):
            M[i, b, :n] = np.asarray(x, dtype=np.float64)[:n].astype(np.float32)
    assert nlay.max() == Lmax and (Lmax == 2 or len(set(nlay)) > 1)                 # ragged wherever a depth allows it
    per = np.array([7.]) if nper == 1 else np.geomspace(2., 40., nper)
    c = np.tile([np.nan, 1e30, 123.0], per.size + PAD)[:per.size + PAD] * np.ones((B, 1))
    for b in range(B):
        r = twin.phase.sensitivity(*[M[i, b, :nlay[b]] for i in range(4)], per, wave)
        assert r['err'] == 0 and np.all(r['c0'] > 0), (name, b)
        c[b, :per.size] = r['c0']
    err = np.zeros((B, 2), dtype=np.int32)
    err[:, 1] = 5                                                                    # another target's flags
    M[2, 0, 0] = 0.0                                                                 # water on top
    err[2, 0] = 1                                                                    # the search's flag
    c[3, 0] = 0.0                                                                    # c_zero: that period only
    c[4, per.size - 1] *= 1 + 1e-5                                                   # c_moved: the polish is rejected
    nlay[B - 1] = 1                                                                  # a half-space alone, in the partial block
    nlay[B - 2] = Lmax + 1                                                           # not a model of this depth: nothing is read
    want = [np.array(x) for x in zip(*[twin.row(*[M[i, b] for i in range(4)], per, c[b, :per.size], wave, nlay=nlay[b],
                                                Lmax=Lmax, err=err[b, 0]) for b in range(B)])]
    _DATA[(name, wave)] = (M, nlay, per, c, err, want)
    return _DATA[(name, wave)]


@pytest.mark.parametrize('wave', ['rayleigh', 'love'])
@pytest.mark.parametrize('name', list(LAYOUTS))
def test_batch_is_the_host_twin_bit_for_bit(lib, twin, name, wave):
    _check_layout(name)
    Lmax, nper, B = LAYOUTS[name]
    M, nlay, per, c, err, want = _layout(twin, name, wave)
    got = _group_batch(lib, M, nlay, per, wave, c, err, Lmax)
    for k, g, w in zip(OUT, got, want):
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), k
    K, U, dU, co, Kp = got
    for b in (0, 2, B - 2, B - 1):                                                   # NaN together
        assert all(np.isnan(x[b]).all() for x in got), b
    assert all(np.isnan(x[3, 0]).all() and np.isnan(x[4, nper - 1]).all() for x in got)
    live = [b for b in range(B) if b not in (0, 2, 3, 4, B - 2, B - 1)]
    assert all(np.isfinite(x[live]).all() for x in got)
    if nper > 1:
        assert np.isfinite(K[3, 1:]).all() and np.isfinite(K[4, :-1]).all()
    for b in live:
        n = nlay[b]
        assert np.all(K[b, :, :, n:] == 0) and np.all(K[b, :, 0, n - 1] == 0) and np.any(K[b, :, 2, :n] != 0)
    if wave == 'love':
        assert np.all(K[live][:, :, 1, :] == 0)
    # K_phase and c are the phase pass's bits, and K_phase may be left out
    Kc, cc, _ = _phase_batch(lib, M, nlay, per, wave, c, err, Lmax)
    ok = ~np.isnan(co)
    assert ok.any() and np.array_equal(co[ok], cc[ok]) and np.array_equal(Kp[ok], Kc[ok])
    assert np.isfinite(cc[~ok]).sum() == 0                       # (no side root is rejected here: the same rows have no value)
    without = _group_batch(lib, M, nlay, per, wave, c, err, Lmax, k_phase=False)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(without[:4], got[:4])) and np.all(without[4] == -777.0)


def test_a_drawn_batch_loses_no_period_the_phase_pass_serves(lib, twin):
    """64 ten-layer draws (the models of tools/sens_group_bench.py), the ten of sens_group_tolerances.DRAWN_LOST among
    them, 21 periods, Rayleigh: every (model, period) the phase pass has a value for has a group value, bit for bit the
    twin's."""
    import sens_group_tolerances as gtol
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(3072, 10, seed=1)
    rows = (list(range(54)) + sorted(gtol.DRAWN_LOST))
    per = np.linspace(1., 41., 21)
    M = np.stack([x[rows, :10].astype(np.float32).astype(np.float64) for x in (H, VP, VS, RHO)])
    nlay = nl[rows].astype(np.int32)
    c = np.array([twin.phase.sensitivity(*[M[i, b] for i in range(4)], per, 'rayleigh')['c0'] for b in range(len(rows))])
    err = np.zeros((len(rows), 1), dtype=np.int32)
    got = _group_batch(lib, M, nlay, per, 'rayleigh', c, err, 10)
    Kc, cc, _ = _phase_batch(lib, M, nlay, per, 'rayleigh', c, err, 10)
    assert np.isfinite(cc).all() and np.isfinite(Kc).all()
    assert all(np.isfinite(x).all() for x in got) and np.array_equal(got[3], cc) and np.array_equal(got[4], Kc)
    want = [np.array(x) for x in zip(*[twin.row(*[M[i, b] for i in range(4)], per, c[b], 'rayleigh') for b in range(len(rows))])]
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize('wave,ref_name', [('rayleigh', 'rdispgr'), ('love', 'ldispph')])
def test_single_model_forms_are_the_twins_search_and_pass(lib, twin, wave, ref_name):
    from bayhunter_amd import plugins
    for name in ('L2', 'L8', 'lvz'):
        m = sc.MODELS[name]
        want = twin.sensitivity(*m, sc.PERIODS, wave)
        f = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)) for x in m]
        n = len(f[0])
        K, Kp, err = np.zeros((5, 4, n)), np.zeros((5, 4, n)), C.c_int(-1)
        U, dU, c = np.zeros(5), np.zeros(5), np.zeros(5)
        assert lib.bh_group_sensitivity(*[x.ctypes.data for x in f], n, 0, sc.WAVES[wave], 5, sc.PERIODS.ctypes.data,
                                        K.ctypes.data, U.ctypes.data, dU.ctypes.data, c.ctypes.data, Kp.ctypes.data,
                                        C.byref(err)) == 0
        assert err.value == 0
        for k, g in zip(OUT, (K, U, dU, c, Kp)):
            assert np.array_equal(g, want[k]), k
        # the batch of one, on the search's own phase velocities
        M = np.stack([x.astype(np.float64)[None, :] for x in f])
        one = _group_batch(lib, M, np.array([n], dtype=np.int32), sc.PERIODS, wave, want['c0'][None, :],
                           np.zeros((1, 1), dtype=np.int32), n)
        for k, g in zip(OUT, one):
            assert np.array_equal(g[0], want[k]), k
        got = plugins.SurfDisp(sc.PERIODS, ref_name).group_sensitivity(*m)
        assert sorted(got) == sorted(OUT) and all(np.array_equal(got[k], want[k]) for k in OUT)
    bad = plugins.SurfDisp(sc.PERIODS, ref_name).group_sensitivity([1., 0.], [np.nan, 6.], [np.nan, 3.5], [2.5, 2.8])
    assert all(np.isnan(bad[k]).all() for k in OUT)


def test_engine_group_sensitivity_on_a_group_target_is_the_call_on_an_equal_phase_target(lib, twin):
    import torch
    from bayhunter_amd import sensitivity as S
    from bayhunter_amd.engine import ForwardEngine, SwdSpec
    M, nlay, per, _, _, _ = _layout(twin, '16x5x7', 'rayleigh')
    keep = [b for b in range(nlay.size) if 2 <= nlay[b] <= 16 and b != 0]
    Mz = np.where(np.arange(16)[None, None, :] < nlay[keep][None, :, None], M[:, keep, :16], 0.0)
    nl = nlay[keep].copy()
    alone = ForwardEngine(swd=[SwdSpec('rdispgr', per)])                       # a group target alone: the companion engine
    both = ForwardEngine(swd=[SwdSpec('rdispgr', per), SwdSpec('ldispgr', per), SwdSpec('rdispph', per)])
    phase = ForwardEngine(swd=[SwdSpec('rdispph', per)])
    res = {}
    for key, eng, target in (('alone', alone, 0), ('equal', both, 0), ('own', both, 2), ('phase', phase, 0)):
        models = eng.upload(*Mz, nl)
        out, err = eng.run(models)
        res[key] = {k: v.cpu().numpy() for k, v in eng.group_sensitivity(models, out=out, err=err, target=target).items()}
        torch.cuda.synchronize()
    assert np.isfinite(res['phase']['K']).all() and np.isfinite(res['phase']['U']).all()
    for key in ('alone', 'equal', 'own'):
        for k in OUT:
            assert res[key][k].tobytes() == res['phase'][k].tobytes(), (key, k)
    assert len(alone._phase_companions) == 1 and not hasattr(both, '_phase_companions')
    models = both.upload(*Mz, nl)
    love = {k: v.cpu().numpy() for k, v in both.group_sensitivity(models, target=1).items()}       # its own companion, Love
    assert np.all(love['K'][:, :, 1, :] == 0) and np.isfinite(love['U']).all() and list(both._phase_companions) == [1]
    models = alone.upload(*Mz, nl)
    # the refusals of the phase entry point stay, and the group one refuses what neither serves
    with pytest.raises(ValueError, match='group-velocity targets are not served'):
        alone.sensitivity(models, target=0)
    hm = ForwardEngine(swd=[SwdSpec('rdispgr', per, 2)])
    with pytest.raises(ValueError, match='mode'):
        hm.group_sensitivity(hm.upload(*Mz, nl))
    # the stand-alone form
    gb = S.group_batch(per, *Mz, nl, wave='rayleigh')
    assert all(np.array_equal(gb[k], res['phase'][k]) for k in OUT) and np.all(gb['err'] == 0)


# ---- pools ------------------------------------------------------------------------------------------------------------------
ARRAYS = ('mean', 'std', 'min', 'max', 'halfspace_mean', 'halfspace_std', 'nmodels', 'nexcluded')


def same_result(one, other):
    assert sorted(one) == sorted(other)
    for k in one:
        a, b = np.asarray(one[k]), np.asarray(other[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def restatement(pool, ci, ri, w, periods, edges):
    """Per row the binned kernel from sensitivity.group_batch + vs_total + to_depth -> (x [rows, nper, bins + 1] float64
    with the half-space last, counts [rows, nper], Lmax)."""
    import torch
    from bayhunter_amd import datafits as df, sensitivity as sens
    from bayhunter_amd.models import layers_from_voronoi
    rows = torch.from_numpy(pool.models[ci, ri].astype(np.float64)).cuda()
    vsn, zv, nl = df._layers(rows, rows.device)
    dm, _ = layers_from_voronoi(vsn, zv, nl, torch.from_numpy(pool.vpvs[ci, ri].astype(np.float64)).cuda(), df._OPEN_PRIORS,
                                mantle=pool.priors.get('mantle'))
    H, VP, VS, RHO = (dm.packed[:, k, :].cpu().numpy() for k in range(4))
    nlay = dm.nlay.cpu().numpy()
    res = sens.group_batch(periods, H, VP, VS, RHO, nlay, 'rayleigh')
    with np.errstate(invalid='ignore', divide='ignore'):
        G = sens.vs_total(res['K'], (VP / VS)[:, None, :])
    x = np.zeros((ci.size, periods.size, edges.size))
    for r in range(ci.size):
        n = int(nlay[r])
        if n >= 2:
            x[r, :, :-1], x[r, :, -1] = sens.to_depth(G[r][:, :n], H[r, :n], edges)
    return x, (w > 0)[:, None] & (nlay >= 2)[:, None] & ~np.isnan(res['U']), H.shape[1]


def test_chain_pool_group_sensitivity_lies_within_the_bounds_of_the_restatement(lib):
    from bayhunter_amd import sensitivity as sens
    from bayhunter_amd.chains import GpuEvaluator
    from bayhunter_amd.selection import pool_rows
    from bayhunter_amd.chains import ChainPool
    from chain_scenario import CASES, joint_target
    # chain_scenario.make_pool's pool of test_gpu_pool_sensitivity's refusal, with storage for every iteration: so short
    # a chain accepts more than the default iterations * max(acceptance) / 100 rows
    case = CASES['tutorial']
    joint = joint_target(DATA, refs=('rdispgr', 'prf'))
    with ChainPool(joint, initparams=dict(case['initparams'], iter_burnin=20, iter_main=10), modelpriors=case['priors'],
                   seeds=[1, 2], evaluator=GpuEvaluator(joint), nmodels=31) as pool:
        pool.run()
        with pytest.raises(ValueError, match='group-velocity targets are not served'):
            pool.sensitivity()                                                      # the phase entry point still refuses
        got = pool.group_sensitivity(dev=0.5)
        periods, edges = got['periods'], got['edges']
        assert np.array_equal(periods, pool.targets.targets[0].obsdata.x) and np.array_equal(edges, sens.default_edges())
        assert got['kind'] == 'vs_total' and got['ref'] == 'rdispgr' and got['velocity'] == 'group'
        assert got['mean'].shape == (periods.size, 100)
        ci, ri, w = pool_rows(pool, 'weighted', 0.5, True)
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
            for i, (err, bound) in enumerate(((np.abs(gm - mean), sets_tol.mean_bound(n, Lmax, ab[None, :])[0]),
                                              (np.abs(gs.astype(LD) ** 2 - (sq - mean * mean)),
                                               sets_tol.var_bound(n, Lmax, sq[None, :])[0]))):
                err = err.astype(np.float64)
                worst[i] = max(worst[i], float(np.where(err == 0, 0., err / np.where(err == 0, 1., bound)).max()))
        print('worst error / bound: mean %.3g, variance %.3g' % tuple(worst))
        assert worst[0] <= 1. and worst[1] <= 1., worst
        # no result depends on max_rows; an explicit group ref is the default; the prf target is no dispersion target
        same_result(pool.group_sensitivity(dev=0.5, max_rows=7), got)
        same_result(pool.group_sensitivity(ref='rdispgr', dev=0.5), got)
        with pytest.raises(ValueError, match='no dispersion target'):
            pool.group_sensitivity(ref='ldispgr')


def test_station_pool_group_sensitivity_equals_every_station_view(lib):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=20, iter_main=10)
    stations = make_stations(DATA, 3, refs=('rdispgr', 'prf'), yerr=True)
    with StationPool(dict(zip(['AAA', 'BBB', 'CCC'], stations)), ip, case['priors'], chains_per_station=2,
                     random_seeds=[51, 52, 53], nmodels=31) as pool:
        pool.run()
        res = pool.group_sensitivity(dev=0.5)
        assert res.names == ['AAA', 'BBB', 'CCC'] and not res.failed and sorted(res.stations) == res.names
        assert res.ref == 'rdispgr' and res.velocity == 'group'
        for s, name in enumerate(res.names):
            one = pool.station(name).group_sensitivity(dev=0.5)                # ChainPool.group_sensitivity on the view
            same_result(res.stations[name], one)
            assert one['velocity'] == 'group' and one['nmodels'].min() > 0 and np.all(one['min'] <= one['max'])
            for k in ARRAYS:
                assert getattr(res, k)[s].tobytes() == one[k].tobytes(), (name, k)
        assert not np.array_equal(res.mean[0], res.mean[1])
