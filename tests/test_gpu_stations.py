"""Station pool on the GPU (bayhunter_amd/stations.py, bh_likelihood_sets, bh_eval_set_observations).

Every equality here is exact: a model's forward row and likelihood do not depend on the batch it is in (all kernel
forms are bit-identical, tests/test_likelihood.py::test_gpu_gauss_form_does_not_depend_on_the_batch), so the chains
of a station inside a pool of many are the chains of a ChainPool of that station alone, and the multi-set
likelihood of a row is what bh_likelihood_batch gives for it with its own set's observations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
from chain_scenario import CASES  # noqa: E402
from station_scenario import make_stations  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, 'tutorial_observed')
KEYS = ('models', 'likes', 'misfits', 'noise', 'vpvs', 'iter')


def _params(name, burnin=None, main=None):
    case = CASES[name]
    burnin, main = burnin or case['burnin'], main or case['main']
    return dict(case['initparams'], iter_burnin=burnin, iter_main=main), case['priors'], burnin + main + 1


def _stations(name, S, yerr, use_mfma=True):
    st = make_stations(DATA, S, refs=CASES[name].get('refs', ('rdispph', 'prf')), yerr=yerr)
    for j in st:
        j.use_mfma = use_mfma
    return st


def _assert_same_chains(view, single):
    for k in KEYS:
        assert np.array_equal(getattr(view, k), getattr(single, k), equal_nan=True), k
    for a, b in zip(view.counters(), single.counters()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('name', sorted(CASES))
def test_gpu_golden_station_inside_a_pool_of_three(golden_chains, name):
    """The committed golden set-ups (chains of the reference's own SingleChain) as station 0 of three: what
    test_gpu_pool_reproduces_reference_chains asserts for a pool of that station alone holds inside the station
    pool, and all three stations equal their single-station pools.  Covariance models: tutorial GAUSS + NOCORR,
    constrained EXP + NOCORR, fixednoise NOCORR, sixtargets EXP."""
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool
    ip, priors, nmodels = _params(name)
    gseeds = [int(s) for s in golden_chains['%s/seeds' % name]]
    c = len(gseeds)
    seeds = [gseeds, [(s * 7 + 1) % 1000 for s in gseeds], [(s * 13 + 2) % 1000 for s in gseeds]]
    with StationPool(_stations(name, 3, False), ip, priors, seeds=seeds, groups=2, nmodels=nmodels) as pool:
        pool.run()
        assert len(pool.pool.groups) == 2 and pool.nchains == 3 * c
    view = pool.station(0)
    for i, seed in enumerate(gseeds):
        got = view.chain(i)
        ref = {k: golden_chains['%s/%d/%s' % (name, seed, k)] for k in KEYS + ('n',)}
        assert got['n'] == int(ref['n']), (name, seed)
        for k in ('models', 'noise', 'vpvs', 'iter'):
            assert np.array_equal(ref[k], got[k], equal_nan=True), (name, seed, k)
        # float32 rows of float64 values that agree to ~1e-12: at most one float32 ulp apart
        assert np.allclose(ref['likes'], got['likes'], rtol=3e-7, atol=0), (name, seed)
        assert np.allclose(ref['misfits'], got['misfits'], rtol=3e-7, atol=0), (name, seed)
        assert np.mean(ref['likes'] == got['likes']) > 0.99
    for s, joint in enumerate(_stations(name, 3, False)):
        with ChainPool(joint, ip, priors, seeds=seeds[s], nmodels=nmodels) as single:
            single.run()
        _assert_same_chains(pool.station(s), single)
    assert not np.array_equal(pool.station(1).likes[:, 0], pool.station(2).likes[:, 0])


@pytest.mark.parametrize('use_mfma', [True, False], ids=['mfma', 'vector'])
def test_gpu_scaled_and_gauss_stations_equal_single_pools(use_mfma):
    """yerr-scaled dispersion noise (every station its own yerr: per-set scaled errors and log-determinant) with the
    dense Gaussian receiver-function noise, on the matrix cores and on the vector units; with random_seeds, a
    look-ahead and a group boundary inside station 2 (chain 10 of 5 x 4)."""
    from bayhunter_amd import _lib
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool
    ip, priors, nmodels = _params('tutorial', 80, 40)
    rs = [3, 1, 4, 15, 9]
    with StationPool(_stations('tutorial', 5, True, use_mfma), ip, priors, chains_per_station=4, random_seeds=rs, groups=2,
                     lookahead=5, nmodels=nmodels) as pool:
        pool.run()
    assert [t.covmodel for t in pool.stations[0].targets] == [_lib.COV_NOCORR_SCALED, _lib.COV_GAUSS]
    assert [(g.first, g.last) for g in pool.pool.groups] == [(0, 10), (10, 20)]
    likes0 = []
    for s, joint in enumerate(_stations('tutorial', 5, True, use_mfma)):
        with ChainPool(joint, ip, priors, random_seed=rs[s], nchains=4, nmodels=nmodels) as single:
            single.run()
        _assert_same_chains(pool.station(s), single)
        likes0.append(float(single.likes[0, 0]))
    assert len(set(likes0)) == 5


def test_gpu_many_stations_share_the_waves_of_the_gauss_product():
    """40 stations x 4 chains: a wave of gauss_q_kernel (16 models) holds rows of four and more stations, a
    like_kernel workgroup (8 models) rows of two or more.  Every station equals its own ChainPool; so does a pool of
    one station."""
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool
    ip, priors, nmodels = _params('tutorial', 40, 20)
    S, c = 40, 4
    rs = list(range(50, 50 + S))
    with StationPool(_stations('tutorial', S, True), ip, priors, chains_per_station=c, random_seeds=rs,
                     nmodels=nmodels) as pool:
        pool.run()
    assert pool.nchains == 160 and len(pool.pool.groups) == 2 and pool.pool.lookahead > 1
    stations = _stations('tutorial', S, True)
    for s in range(S):
        with ChainPool(stations[s], ip, priors, random_seed=rs[s], nchains=c, nmodels=nmodels) as single:
            single.run()
        _assert_same_chains(pool.station(s), single)
    with StationPool(stations[:1], ip, priors, chains_per_station=c, random_seeds=rs[:1], nmodels=nmodels) as one:
        one.run()
    _assert_same_chains(one.station(0), pool.station(0))
    _assert_same_chains(one.pool, pool.station(0))


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
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind in 'fc' else np.array_equal(x, y), path


def test_gpu_station_views_feed_the_post_processing(tmp_path):
    """posterior() / datafits() / outliers() of a station view equal those of the single-station pool; save() writes
    the single-station pool's .npy files byte for byte."""
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool
    ip, priors, nmodels = _params('tutorial', 150, 100)
    rs = [21, 22, 23]
    with StationPool(_stations('tutorial', 3, True), ip, priors, chains_per_station=4, random_seeds=rs,
                     nmodels=nmodels) as pool:
        pool.run()
    pool.save(str(tmp_path / 'all'))
    for s, joint in enumerate(_stations('tutorial', 3, True)):
        with ChainPool(joint, ip, priors, random_seed=rs[s], nchains=4, nmodels=nmodels) as single:
            single.run()
        view = pool.station(s)
        assert np.array_equal(view.outliers(), single.outliers())
        _assert_equal_trees(view.posterior(dev=0.5), single.posterior(dev=0.5), 'posterior')
        _assert_equal_trees(view.datafits(dev=0.5), single.datafits(dev=0.5), 'datafits')
        single.save(str(tmp_path / ('one%d' % s)))
        mine, ref = tmp_path / 'all' / pool.names[s] / 'data', tmp_path / ('one%d' % s) / 'data'
        files = sorted(f for f in os.listdir(str(ref)) if f.endswith('.npy'))
        assert files == sorted(f for f in os.listdir(str(mine)) if f.endswith('.npy')) and len(files) >= 20
        for f in files:
            assert (mine / f).read_bytes() == (ref / f).read_bytes(), (s, f)


# ---- the likelihood entry point ---------------------------------------------------------------------------
def _like_case(n, B, nsets=7):
    """Row = [21 yerr-scaled | 30 exponential | 10 diagonal | n dense Gaussian] columns + 2 spare; random modelled
    data, noise, observations and errors per set, one (asymmetric) R^-1 for all sets."""
    from bayhunter_amd import _lib
    rs = np.random.RandomState(1000 * n + B % 1000)
    row = 61 + n + 2
    out = rs.normal(size=(B, row))
    noise = np.stack([rs.uniform(0.1, 0.9, B), rs.uniform(0.5, 2.0, B)] * 4, axis=1)
    yobs = rs.normal(size=(nsets, row))
    scale = np.ones((nsets, row))
    scale[:, :21] = rs.uniform(1.0, 4.0, size=(nsets, 21))
    logdet = np.zeros((nsets, 4))
    logdet[:, 0] = np.log(np.prod(scale[:, :21], axis=1))
    Rinv = (rs.normal(size=(n, n)) / n).ravel()
    obs_id = rs.randint(0, nsets, B).astype(np.int32)

    def desc(s):      # the descriptors of set s alone: scaled errors at aux[0:21], R^-1 behind them
        return (_lib.LikeTarget * 4)(_lib.LikeTarget(21, 0, _lib.COV_NOCORR_SCALED, 0, float(logdet[s, 0])),
                                     _lib.LikeTarget(30, 21, _lib.COV_EXP, 0, 0.0),
                                     _lib.LikeTarget(10, 51, _lib.COV_NOCORR, 0, 0.0),
                                     _lib.LikeTarget(n, 61, _lib.COV_GAUSS, 21, 0.75))
    aux = [np.concatenate([scale[s, :21], Rinv]) for s in range(nsets)]
    return dict(row=row, out=out, noise=noise, yobs=yobs, scale=scale, logdet=logdet, obs_id=obs_id, desc=desc, aux=aux)


@pytest.mark.parametrize('n,B', [(16, 300), (60, 1000), (201, 3000), (256, 777), (201, 40000), (60, 33000), (16, 40000),
                                 (256, 34000)])
def test_gpu_likelihood_sets_equal_one_call_per_set(lib, n, B):
    """bh_likelihood_sets over 7 sets = bh_likelihood_batch once per set on that set's rows, row by row and bit for
    bit: with the workspace (SPLIT form up to 32 768 rows, fused form above) in one call and as two stages, and
    without it (vector units).  obs_id = NULL with one set is the existing call.  An index out of range gives the
    failed-model result for that row and leaves its neighbours alone."""
    import torch
    from bayhunter_amd import _lib
    k = _like_case(n, B)
    dev = torch.device('cuda')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    row, T = k['row'], 4
    t_out, t_noise = up(k['out']), up(k['noise'])
    t_yobs, t_scale, t_logdet = up(k['yobs']), up(k['scale']), up(k['logdet'])
    t_aux0 = up(k['aux'][0])
    need = lib.bh_likelihood_workspace_bytes(B, T, k['desc'](0))
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)

    def sets(obs_id, stages=(3,), use_ws=True, nsets=7, tables=True):
        t_id = None if obs_id is None else up(obs_id)
        logL = torch.full((B,), 7.0, dtype=torch.float64, device=dev)
        mis = torch.full((B, T + 1), 7.0, dtype=torch.float64, device=dev)
        for st in stages:
            _lib.check(lib.bh_likelihood_sets(
                st, B, T, k['desc'](0), t_out.data_ptr(), row, None, 0, nsets, None if t_id is None else t_id.data_ptr(),
                t_yobs.data_ptr(), row, t_scale.data_ptr() if tables else None, t_logdet.data_ptr() if tables else None,
                t_noise.data_ptr(), t_aux0.data_ptr(), logL.data_ptr(), mis.data_ptr(), ws.data_ptr() if use_ws else None,
                need if use_ws else 0, None))
        torch.cuda.synchronize()
        return logL.cpu().numpy(), mis.cpu().numpy()

    def per_set(use_ws=True):
        logL, mis = np.zeros(B), np.zeros((B, T + 1))
        for s in range(7):
            sel = np.nonzero(k['obs_id'] == s)[0]
            nb = sel.size
            assert nb > 0
            o, z, y, a = up(k['out'][sel]), up(k['noise'][sel]), up(k['yobs'][s]), up(k['aux'][s])
            nd = lib.bh_likelihood_workspace_bytes(nb, T, k['desc'](s))
            w = torch.empty(nd // 8, dtype=torch.float64, device=dev)
            ll = torch.zeros(nb, dtype=torch.float64, device=dev)
            mm = torch.zeros((nb, T + 1), dtype=torch.float64, device=dev)
            _lib.check(lib.bh_likelihood_batch(nb, T, k['desc'](s), o.data_ptr(), row, None, 0, y.data_ptr(), z.data_ptr(),
                                               a.data_ptr(), ll.data_ptr(), mm.data_ptr(), w.data_ptr() if use_ws else None,
                                               nd if use_ws else 0, None))
            torch.cuda.synchronize()
            logL[sel], mis[sel] = ll.cpu().numpy(), mm.cpu().numpy()
        return logL, mis
    want_l, want_m = per_set()
    assert np.isfinite(want_l).all()
    got_l, got_m = sets(k['obs_id'])
    assert np.array_equal(got_l, want_l) and np.array_equal(got_m, want_m)
    got_l, got_m = sets(k['obs_id'], stages=(1, 2))                     # the two stages separately
    assert np.array_equal(got_l, want_l) and np.array_equal(got_m, want_m)
    if B <= 3000:                                                       # the vector-unit product (no workspace)
        vec_l, vec_m = per_set(use_ws=False)
        got_l, got_m = sets(k['obs_id'], use_ws=False)
        assert np.array_equal(got_l, vec_l) and np.array_equal(got_m, vec_m)
    # one set, no index: the existing call (tables or aux for the scaled errors: the same numbers)
    o_l = torch.zeros(B, dtype=torch.float64, device=dev)
    o_m = torch.zeros((B, T + 1), dtype=torch.float64, device=dev)
    _lib.check(lib.bh_likelihood_batch(B, T, k['desc'](0), t_out.data_ptr(), row, None, 0, t_yobs.data_ptr(),
                                       t_noise.data_ptr(), t_aux0.data_ptr(), o_l.data_ptr(), o_m.data_ptr(), ws.data_ptr(),
                                       need, None))
    torch.cuda.synchronize()
    for tables in (False, True):
        got_l, got_m = sets(None, nsets=1, tables=tables)
        assert np.array_equal(got_l, o_l.cpu().numpy()) and np.array_equal(got_m, o_m.cpu().numpy())
    # indices out of range: the failed-model result for those rows, everything else untouched
    bad = k['obs_id'].copy()
    where = np.array([0, 5, 17, 18, B // 2, B - 1])
    bad[where] = [7, -1, 2 ** 30, -2 ** 31, 7, 100]
    got_l, got_m = sets(bad)
    keep = np.ones(B, dtype=bool)
    keep[where] = False
    assert np.all(got_l[where] == -1e15) and np.all(got_m[where] == 1e15)
    assert np.array_equal(got_l[keep], want_l[keep]) and np.array_equal(got_m[keep], want_m[keep])


def test_gpu_plan_observations_lifecycle_and_refusals():
    """bh_eval_set_observations on a live plan: once, before the first submit, with tables when a target is
    yerr-scaled; bh_eval_submit refuses a chain number outside set_of_chain."""
    from bayhunter_amd import _lib
    from bayhunter_amd.stations import observation_tables
    st = _stations('tutorial', 3, True)
    for j in st:
        j.set_target_covariance([True, True], [0.0, 0.9], 1e-5)
    yobs, scale, logdet = observation_tables(st)
    assert scale is not None and yobs.shape == (3, 222) and logdet.shape == (3, 2)
    soc = np.array([0, 0, 1, 2], dtype=np.int32)
    with st[0].eval_plan(16, 12) as plan:
        with pytest.raises(_lib.BayHunterAmdError, match='BH_COV_NOCORR_SCALED'):
            plan.set_observations(yobs, soc)
        plan.set_observations(yobs, soc, scale, logdet)
        with pytest.raises(_lib.BayHunterAmdError, match='already'):
            plan.set_observations(yobs, soc, scale, logdet)
        plan.packed[:4] = 0.0
        plan.packed[:4, 0, 0], plan.packed[:4, 1, :2], plan.packed[:4, 2, :2], plan.packed[:4, 3, :2] = 30., 6., 3.5, 2.7
        plan.nlay[:4] = 2
        plan.noise[:4] = [0.0, 0.02, 0.9, 0.01]
        plan.chain[:4] = [0, 1, 2, 3]
        plan.submit(4)
        logL = plan.wait()[0].copy()
        assert logL[0] == logL[1] and len(set(logL[1:])) == 3           # chains 0 and 1 share station 0
        plan.chain[2] = 4
        with pytest.raises(_lib.BayHunterAmdError, match='chain'):
            plan.submit(4)
    with st[0].eval_plan(16, 12) as plan:
        plan.submit(0)
        with pytest.raises(_lib.BayHunterAmdError, match='after bh_eval_submit'):
            plan.set_observations(yobs, soc, scale, logdet)


def test_gpu_station_pools_made_run_and_closed_back_to_back():
    """Station pools (two plans each, every plan with its observation tables) made, run and closed one after the
    other in one process, under `with` and with explicit close() (tests/scenarios/station_lifecycle.py; a child
    process: a failure here could as well be a crash)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'scenarios', 'station_lifecycle.py'), '5', '48', '8', '40'],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec['ok'] and rec['pools'] == 5 and rec['plans_closed'] == 10 and rec['same_chains'] == 5
