"""Stations with data gaps on the GPU: like_gaps_kernel through bh_likelihood_sets_gaps, bh_eval_set_gaps and
StationPool(missing='mask').

The masked call is defined by the compacted one: a row's logL and misfits are, bit for bit, those of a
bh_likelihood_stage call whose target table, `out` rows and yobs hold the kept columns of the row's set -- lane i of
a wave takes elements i, i + 64, ... of the compacted vector in both.  The same rows are judged against the
extended-precision evaluation of the compacted arrays with likelihood_hp's own bounds for n' samples."""
import os
import sys

import numpy as np
import pytest

import likelihood_hp as hp
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
from chain_scenario import CASES  # noqa: E402
from station_scenario import make_stations  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(GOLDEN, 'tutorial_observed')
KEYS = ('models', 'likes', 'misfits', 'noise', 'vpvs', 'iter')
SHAPES = [(300, 65), (17, 65), (300, 129)]      # 17: a partial last workgroup; 129: three strides of a wave
NG = 16                                         # the dense target, which has no gaps
_CACHE = {}


def build(B, n):
    """One target each of NOCORR, SCALED and EXP with n samples and a GAUSS target with 16, three sets: set 0 full,
    set 1 with gaps at both ends and a run in the middle, set 2 random and with ONE kept sample of the EXP target.
    What a gap's column holds in out, yobs and set_scale is finite and absurd: it must not be read."""
    if (B, n) in _CACHE:
        return _CACHE[(B, n)]
    rs = np.random.RandomState(100 * n + B)
    covs, ns, offs = (hp.COV_NOCORR, hp.COV_NOCORR_SCALED, hp.COV_EXP, hp.COV_GAUSS), (n, n, n, NG), []
    pos = 1
    for k in ns:
        offs.append(pos)
        pos += k + 2
    stride, nsets, T = pos + 1, 3, 4
    present = np.ones((nsets, stride), dtype=np.uint8)
    for t in range(3):
        m = np.ones(n, dtype=np.uint8)
        m[[0, n - 1]] = 0
        m[n // 3:n // 3 + 7 + t] = 0
        present[1, offs[t]:offs[t] + n] = m
        m = (rs.uniform(size=n) > 0.35).astype(np.uint8)
        m[rs.randint(n)] = 1
        present[2, offs[t]:offs[t] + n] = m
    one = np.zeros(n, dtype=np.uint8)
    one[n - 2] = 1
    present[2, offs[2]:offs[2] + n] = one
    gap = present == 0
    yobs = rs.standard_normal((nsets, stride))
    obs_id = rs.randint(0, nsets, B).astype(np.int32)
    obs_id[:3] = [2, 0, 1]
    out = yobs[obs_id] + rs.standard_normal((B, stride)) * 10.0 ** rs.uniform(-3, 0, B)[:, None]
    out[gap[obs_id]] = -3e30
    yobs[gap] = 1e30
    yerr = rs.uniform(0.01, 0.04, (nsets, stride))
    scale, logdet = np.full((nsets, stride), 7.0), np.zeros((nsets, T))
    for s in range(nsets):
        keep = offs[1] + np.nonzero(present[s, offs[1]:offs[1] + n])[0]
        scale[s, keep] = yerr[s, keep] / yerr[s, keep].min()
        logdet[s, 1] = np.log(np.prod(scale[s, keep]))
    noise = np.empty((B, 2 * T))
    noise[:, 0::2], noise[:, 1::2] = rs.uniform(-0.95, 0.95, (B, T)), rs.uniform(0.005, 2.0, (B, T))
    noise[:5, 4] = hp.CORRS[-5:]
    rinv = hp.dense_matrix('pinv0.98', NG).ravel()
    targets = [hp.Target(k, off, cov, 0, 1.75 if cov == hp.COV_GAUSS else 0.0) for k, off, cov in zip(ns, offs, covs)]
    err = np.zeros((B, 1), dtype=np.int32)
    err[B // 2, 0] = 3                                                  # one failed model
    k = dict(B=B, n=n, T=T, stride=stride, nsets=nsets, targets=targets, present=present, yobs=yobs, obs_id=obs_id, out=out,
             scale=scale, logdet=logdet, noise=noise, aux=rinv, err=err)
    k['compact'] = [compact(k, s) for s in range(nsets)]
    _CACHE[(B, n)] = k
    return k


def compact(k, s):
    """Set s as a data file without the missing lines: the rows of the set, a target table of n' samples each, out and
    yobs with the kept columns only, the scaled errors in aux -- the arguments of bh_likelihood_stage."""
    rows = np.nonzero(k['obs_id'] == s)[0]
    cols, targets, aux, pos, aux_off = [], [], [], 0, 0
    for t, tg in enumerate(k['targets']):
        keep = tg.off + np.nonzero(k['present'][s, tg.off:tg.off + tg.n])[0]
        extra, a_off = tg.logdet_extra, 0
        if tg.cov == hp.COV_NOCORR_SCALED:
            aux.append(k['scale'][s, keep])
            extra, a_off = float(k['logdet'][s, t]), aux_off
            aux_off += keep.size
        elif tg.cov == hp.COV_GAUSS:
            aux.append(k['aux'])
            a_off = aux_off
            aux_off += k['aux'].size
        targets.append(hp.Target(keep.size, pos, tg.cov, a_off, extra))
        cols.append(keep)
        pos += keep.size
    cols = np.concatenate(cols)
    return dict(rows=rows, targets=targets, aux=np.ascontiguousarray(np.concatenate(aux)), stride=pos,
                out=np.ascontiguousarray(k['out'][rows][:, cols]), yobs=np.ascontiguousarray(k['yobs'][s, cols]),
                noise=np.ascontiguousarray(k['noise'][rows]), err=np.ascontiguousarray(k['err'][rows]))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _call(lib, mode, targets, B, fn):
    """fn(stage, logL, mis, ws, ws_bytes) -> rc, once per stage of `mode` -> (logL, mis) on the host."""
    import torch
    from bayhunter_amd import _lib
    T = len(targets)
    desc = (_lib.LikeTarget * T)(*[_lib.LikeTarget(*tg) for tg in targets])
    need = lib.bh_likelihood_workspace_bytes(B, T, desc)
    ws = torch.full((max(need // 8, 1),), float('nan'), dtype=torch.float64, device='cuda')
    wsp, wsn = (ws.data_ptr(), need) if mode != 'nows' else (None, 0)
    logL = torch.full((B,), float('nan'), dtype=torch.float64, device='cuda')
    mis = torch.full((B, T + 1), float('nan'), dtype=torch.float64, device='cuda')
    for st in ((1, 2) if mode == 'staged' else (3,)):
        _lib.check(fn(st, desc, logL.data_ptr(), mis.data_ptr(), wsp, wsn))
    torch.cuda.synchronize()
    return logL.cpu().numpy(), mis.cpu().numpy()


def masked(lib, k, mode, present='table', sets_api=False):
    """bh_likelihood_sets_gaps on the case (present: 'table', 'ones' or None), or bh_likelihood_sets."""
    import torch
    d = {a: _dev(k[a]) for a in ('out', 'yobs', 'noise', 'aux', 'err', 'obs_id', 'scale', 'logdet')}
    gws_bytes = lib.bh_likelihood_gaps_workspace_bytes(k['nsets'], k['stride'], k['T'])
    assert gws_bytes == 4 * (k['nsets'] * k['stride'] + k['nsets'] * k['T'])
    gws = torch.full((gws_bytes // 4,), -1, dtype=torch.int32, device='cuda')
    pres = {'table': k['present'], 'ones': np.ones_like(k['present']), None: None}[present]

    def fn(st, desc, logL, mis, wsp, wsn):
        head = (st, k['B'], k['T'], desc, d['out'].data_ptr(), k['stride'], d['err'].data_ptr(), 1, k['nsets'],
                d['obs_id'].data_ptr(), d['yobs'].data_ptr(), k['stride'], d['scale'].data_ptr(), d['logdet'].data_ptr(),
                d['noise'].data_ptr(), d['aux'].data_ptr(), logL, mis, wsp, wsn)
        if sets_api:
            return lib.bh_likelihood_sets(*head, None)
        return lib.bh_likelihood_sets_gaps(*head, None if pres is None else pres.ctypes.data, gws.data_ptr(), gws_bytes, None)
    return _call(lib, mode, k['targets'], k['B'], fn)


def staged_compact(lib, c, mode):
    d = {a: _dev(c[a]) for a in ('out', 'yobs', 'noise', 'aux', 'err')}
    B = len(c['rows'])

    def fn(st, desc, logL, mis, wsp, wsn):
        return lib.bh_likelihood_stage(st, B, len(c['targets']), desc, d['out'].data_ptr(), c['stride'], d['err'].data_ptr(), 1,
                                       d['yobs'].data_ptr(), d['noise'].data_ptr(), d['aux'].data_ptr(), logL, mis, wsp, wsn,
                                       None)
    return _call(lib, mode, c['targets'], B, fn)


@pytest.mark.parametrize('B,n', SHAPES)
def test_gpu_masked_call_is_the_compacted_call_bit_for_bit(lib, B, n):
    """For each set, a row's logL and misfits equal those of bh_likelihood_stage on the compacted columns, in every
    mode of likelihood_hp.ALL_MODES; the failed model gets the failed-model result in both."""
    k = build(B, n)
    assert [int(k['present'][2, k['targets'][2].off:][:n].sum()), k['present'][0].all()] == [1, True]
    for mode in hp.ALL_MODES:
        logL, mis = masked(lib, k, mode)
        for s, c in enumerate(k['compact']):
            assert len(c['rows']) > 0 and [t.n for t in c['targets']][3] == NG
            want_l, want_m = staged_compact(lib, c, mode)
            assert logL[c['rows']].tobytes() == want_l.tobytes(), (mode, s)
            assert mis[c['rows']].tobytes() == want_m.tobytes(), (mode, s)
        bad = B // 2
        assert logL[bad] == -1e15 and (mis[bad] == 1e15).all()
        ok = np.arange(B) != bad
        assert np.isfinite(logL[ok]).all() and np.isfinite(mis[ok]).all() and (np.abs(logL[ok]) < 1e14).all()


@pytest.mark.parametrize('B,n', SHAPES)
def test_gpu_masked_call_within_the_extended_precision_bounds(lib, B, n):
    """The same rows against likelihood_hp.evaluate on the compacted arrays, inside its bounds for n' samples."""
    k = build(B, n)
    for mode in hp.ALL_MODES:
        logL, mis = masked(lib, k, mode)
        for s, c in enumerate(k['compact']):
            ref = hp.evaluate(c['out'], c['yobs'], c['noise'], c['aux'], c['targets'], err=c['err'])
            case = dict(rows=np.arange(len(c['rows'])), poisoned=[], case=dict(name='gaps_B%d_n%d_set%d' % (B, n, s)))
            rl, rm, msg = hp.judge(case, logL[c['rows']], mis[c['rows']], ref=ref)
            print('HP-RATIO gpu-gaps %s %s logL=%.3f misfit=%.3f' % (case['case']['name'], mode, rl, rm))
            assert msg is None, (mode, msg)


@pytest.mark.parametrize('B,n', SHAPES[:2])
def test_gpu_full_mask_and_no_mask_are_bh_likelihood_sets(lib, B, n):
    """set_present all ones, and set_present = NULL, give the bytes of bh_likelihood_sets on the same inputs."""
    k = dict(build(B, n))
    k['yobs'] = np.where(k['present'] == 0, 0.25, k['yobs'])           # (all columns are read now: plain numbers)
    k['out'] = np.where(k['present'][k['obs_id']] == 0, 0.5, k['out'])
    for mode in hp.ALL_MODES:
        want_l, want_m = masked(lib, k, mode, sets_api=True)
        for present in ('ones', None):
            logL, mis = masked(lib, k, mode, present=present)
            assert logL.tobytes() == want_l.tobytes() and mis.tobytes() == want_m.tobytes(), (mode, present)
        logL, _ = masked(lib, k, mode)
        assert not np.array_equal(logL, want_l)


# ---- pools ------------------------------------------------------------------------------------------------------
def _params(burnin, main):
    case = CASES['tutorial']
    return dict(case['initparams'], iter_burnin=burnin, iter_main=main), case['priors'], burnin + main + 1


def _gap_stations(S=3):
    """Tutorial stations (21 periods + a receiver function, yerr-scaled dispersion noise); gaps at stations 1 and 2:
    the four shortest periods and, with a sample in the middle, the five longest."""
    st = make_stations(DATA, S, yerr=True)
    assert st[0].targets[0].obsdata.y.size == 21
    for s, miss in ((1, [0, 1, 2, 3]), (2, [9, 16, 17, 18, 19, 20])):
        if s < S:
            y = st[s].targets[0].obsdata.y.copy()
            y[miss] = np.nan
            st[s].targets[0].obsdata.y = y
    return st


def _assert_same_chains(view, single):
    for k in KEYS:
        assert np.array_equal(getattr(view, k), getattr(single, k), equal_nan=True), k
    for a, b in zip(view.counters(), single.counters()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('lookahead', [1, None], ids=['lookahead1', 'default'])
def test_gpu_station_with_gaps_does_not_depend_on_its_pool(lookahead):
    """3 stations x 4 chains, gaps at two stations: station s of the pool equals, bit for bit, the one-station
    StationPool(missing='mask') of station s with the same seeds, and the station without gaps a plain ChainPool."""
    from bayhunter_amd import _lib
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool
    ip, priors, nmodels = _params(150, 100)
    rs = [21, 22, 23]
    with StationPool(_gap_stations(), ip, priors, chains_per_station=4, random_seeds=rs, lookahead=lookahead,
                     nmodels=nmodels, missing='mask') as pool:
        pool.run()
    assert pool.ngaps == 10 and [t.covmodel for t in pool.stations[1].targets] == [_lib.COV_NOCORR_SCALED, _lib.COV_GAUSS]
    assert np.nanmin(pool.pool.likes) > -1e14
    for s in range(3):
        with StationPool([_gap_stations()[s]], ip, priors, chains_per_station=4, random_seeds=rs[s:s + 1],
                         lookahead=lookahead, nmodels=nmodels, missing='mask') as one:
            one.run()
        _assert_same_chains(pool.station(s), one.station(0))
    with ChainPool(make_stations(DATA, 1, yerr=True)[0], ip, priors, random_seed=rs[0], nchains=4, lookahead=lookahead,
                   nmodels=nmodels) as plain:
        plain.run()
    _assert_same_chains(pool.station(0), plain)
    with ChainPool(make_stations(DATA, 2, yerr=True)[1], ip, priors, random_seed=rs[1], nchains=4, lookahead=lookahead,
                   nmodels=nmodels) as complete:
        complete.run()
    assert not np.array_equal(pool.station(1).likes, complete.likes, equal_nan=True)    # the gaps count
    fits = pool.station(1).datafits()['targets'][0]
    assert np.isnan(fits['yobs'][:4]).all() and np.isnan(fits['residual'][:4]).all() and np.isfinite(fits['residual'][4:]).all()
    assert np.isfinite(fits['mean']).all() and np.isfinite(fits['best']).all()


def _fill(plan, n):
    plan.packed[:n] = 0.0
    plan.packed[:n, 0, 0], plan.packed[:n, 1, :2], plan.packed[:n, 2, :2], plan.packed[:n, 3, :2] = 30., 6., 3.5, 2.7
    plan.nlay[:n] = 2
    plan.noise[:n] = [0.0, 0.02, 0.9, 0.01]


def test_gpu_plan_gaps_lifecycle():
    """bh_eval_set_gaps: after the observations, once, before the first submit, nsets that of the observations; a
    plan whose layout has gaps does not run without them; pools made, run and closed back to back leave no error."""
    import torch
    from bayhunter_amd import _lib
    from bayhunter_amd.stations import StationPool, find_gaps, observation_tables
    st = _gap_stations()
    for j in st:
        j.set_target_covariance([True, True], [0.0, 0.9], 1e-5)
    assert find_gaps(['a', 'b', 'c'], st, 'mask') == 10
    yobs, scale, logdet, present = observation_tables(st, present=True)
    soc = np.array([0, 0, 1, 2], dtype=np.int32)
    with st[0].eval_plan(16, 12) as plan:
        with pytest.raises(_lib.BayHunterAmdError, match='bh_eval_set_observations first'):
            plan.set_gaps(present)
        plan.set_observations(yobs, soc, scale, logdet)
        with pytest.raises(_lib.BayHunterAmdError, match=r'nsets = 2.*3 sets'):
            plan.set_gaps(present[:2])
        with pytest.raises(ValueError):
            plan.set_gaps(present[:, :-1])
        dense = present.copy()
        dense[1, -1] = 0                                                  # the receiver function's last sample
        with pytest.raises(_lib.BayHunterAmdError, match=r'set 1, target 1 is BH_COV_GAUSS'):
            plan.set_gaps(dense)
        plan.set_gaps(present)
        with pytest.raises(_lib.BayHunterAmdError, match='already'):
            plan.set_gaps(present)
        _fill(plan, 4)
        plan.chain[:4] = [0, 1, 2, 3]
        plan.submit(4)
        logL, mis = (a.copy() for a in plan.wait())
        with pytest.raises(_lib.BayHunterAmdError, match='after bh_eval_submit'):
            plan.set_gaps(present)
    assert np.isfinite(logL).all() and logL[0] == logL[1] and len(set(logL[1:])) == 3
    with st[1].eval_plan(16, 12) as plan:                                 # a layout with gaps, and no table
        _fill(plan, 1)
        with pytest.raises(_lib.BayHunterAmdError, match='data gaps'):
            plan.submit(1)
    with st[0].eval_plan(16, 12) as plan:                                 # the same rows without the gaps: other numbers
        plan.set_observations(yobs, soc, scale, logdet)
        _fill(plan, 4)
        plan.chain[:4] = [0, 1, 2, 3]
        plan.submit(4)
        shared = plan.wait()[0].copy()
    assert shared[0] == logL[0] and shared[2] != logL[2] and shared[3] != logL[3]
    ip, priors, nmodels = _params(20, 10)
    last = None
    for _ in range(3):
        with StationPool(_gap_stations(), ip, priors, chains_per_station=2, random_seeds=[1, 2, 3], nmodels=nmodels,
                         missing='mask') as pool:
            pool.run()
        assert last is None or np.array_equal(pool.pool.likes, last, equal_nan=True)
        last = pool.pool.likes.copy()
    torch.cuda.synchronize()
    assert _lib.load().bh_stream_synchronize(None) == _lib.BH_OK
