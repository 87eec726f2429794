"""Per-station receiver-function slowness on the GPU: bh_rf_batch_sets (the per-row form of rf_kernel),
bh_eval_set_rf_slowness and StationPool(per_station=('p',)).

Bit identity is the criterion everywhere: a row computed by the per-row form at p = x is the row the uniform form
computes when launched with p = x, NaN positions included, so a station's chains stay those of its own ChainPool.
P receiver functions with p between 4 and 9 s/deg never turn post-critical for the models used here (vp < 10.7 km/s
< 1 / (9 x 0.00899)): every compared row has to be finite, none is skipped."""
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
KEYS = ('models', 'likes', 'misfits', 'noise', 'vpvs', 'iter')


def _assert_same_chains(view, single):
    for k in KEYS:
        assert np.array_equal(getattr(view, k), getattr(single, k), equal_nan=True), k
    for a, b in zip(view.counters(), single.counters()):
        assert np.array_equal(a, b)


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


class _Rf(object):
    """Device copies of a batch of models and the two receiver-function calls on them."""

    def __init__(self, lib, H, VP, VS, RHO, nl, nsamp, waveno, nout=201):
        import torch
        from bayhunter_amd import _lib
        self.lib, self._lib, self.torch = lib, _lib, torch
        self.dev = torch.device('cuda')
        self.B, self.L, self.nout = H.shape[0], H.shape[1], nout
        self.host = (H, VP, VS, RHO, nl)
        self.nsamp, self.waveno = nsamp, waveno

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def par(self, p):
        return self._lib.RfParams(p, 1.0, 5.0, 5.0, -1.0, self.nsamp, self.waveno, self.nout, 0)

    def _run(self, sel, fn):
        H, VP, VS, RHO, nl = (a if sel is None else a[sel] for a in self.host)
        B = H.shape[0]
        d = [self.up(a) for a in (H, VP, VS, RHO)]
        dn = self.up(nl.astype(np.int32))
        out = self.torch.full((B, self.nout), 7.0, dtype=self.torch.float64, device=self.dev)
        self._lib.check(fn(B, dn, d, out))
        self.torch.cuda.synchronize()
        return out.cpu().numpy()

    def uniform(self, p, sel=None):
        return self._run(sel, lambda B, dn, d, out: self.lib.bh_rf_batch(
            B, self.L, self.L, dn.data_ptr(), *[x.data_ptr() for x in d], None, None, self.par(p), out.data_ptr(),
            self.nout, None, 0, None))

    def sets(self, table, set_id, sel=None, par_p=123.0):
        t = self.up(np.asarray(table, dtype=np.float64))
        i = None if set_id is None else self.up(np.asarray(set_id, dtype=np.int32))
        return self._run(sel, lambda B, dn, d, out: self.lib.bh_rf_batch_sets(
            B, self.L, self.L, dn.data_ptr(), *[x.data_ptr() for x in d], None, None, self.par(par_p), len(table),
            t.data_ptr(), None if i is None else i.data_ptr(), out.data_ptr(), self.nout, None, 0, None))


@pytest.mark.parametrize('nsamp', [512, 1024])
@pytest.mark.parametrize('waveno', [0, 1])
@pytest.mark.parametrize('B,layers,Lmax', [(4099, (2, 31), 32), (4099, (2, 12), 12), (5, (2, 12), 12)],
                         ids=['deep', 'shallow', 'five_models'])
def test_gpu_rf_batch_sets_equals_one_uniform_call_per_set(lib, B, layers, Lmax, waveno, nsamp):
    """Ragged models, 7 sets drawn at random: bh_rf_batch_sets = bh_rf_batch once per set on that set's rows, byte for
    byte; par->p is ignored.  2-31 layers in rows of 32, or 1 024 samples: one model per workgroup; 2-12 layers with
    512 samples: three per workgroup, which then belong to different sets, and the last workgroup is partial (4 099
    and 5 are not multiples of three).  An index out of range gives a NaN row and leaves its neighbours alone; no
    index with one set is bh_rf_batch."""
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(B, layers, seed=900 + B + nsamp + waveno + Lmax, Lmax=Lmax)
    rs = np.random.RandomState(17 + B)
    table = np.array([4.0, 9.0, 6.4, 5.25, 7.7, 8.125, 4.9])
    set_id = rs.randint(0, 7, B).astype(np.int32)
    set_id[:min(B, 7)] = np.arange(7)[:min(B, 7)]                       # every set (of the first B) is used
    rf = _Rf(lib, H, VP, VS, RHO, nl, nsamp, waveno)
    want = np.zeros((B, 201))
    for s in np.unique(set_id):
        sel = np.nonzero(set_id == s)[0]
        want[sel] = rf.uniform(float(table[s]), sel)
    if waveno == 0:
        assert np.isfinite(want).all()                                  # (module docstring): nothing to skip
    got = rf.sets(table, set_id)
    assert got.tobytes() == want.tobytes()
    assert len({want[i].tobytes() for i in range(min(B, 7))}) == min(B, 7)
    # one set and no index: the uniform call
    assert rf.sets([6.4], None).tobytes() == rf.uniform(6.4).tobytes()
    # indices out of range
    where = np.array([0, 2, B // 2, B - 1])
    bad = set_id.copy()
    bad[where] = [-1, 7, 2 ** 30, -2 ** 31]
    got = rf.sets(table, bad)
    keep = np.ones(B, dtype=bool)
    keep[where] = False
    assert np.isnan(got[where]).all()
    assert got[keep].tobytes() == want[keep].tobytes()


def test_gpu_rf_batch_sets_post_critical_rows_have_the_uniform_forms_nans(lib):
    """Ray parameters up to 14 s/deg: post-critical for vp > 7.9 km/s.  Incident P: those rows are NaN in both
    forms; incident SV: finite, through the complex form of the recursion.  Equal bytes, hence equal NaN positions."""
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(96, (3, 9), seed=77)
    table = np.array([14.0, 6.4, 11.5])
    set_id = (np.arange(96) % 3).astype(np.int32)
    for waveno in (0, 1):
        rf = _Rf(lib, H, VP, VS, RHO, nl, 512, waveno)
        want = np.zeros((96, 201))
        for s in range(3):
            sel = np.nonzero(set_id == s)[0]
            want[sel] = rf.uniform(float(table[s]), sel)
        got = rf.sets(table, set_id)
        assert got.tobytes() == want.tobytes()
        nan_rows = np.isnan(want).all(axis=1)
        if waveno == 0:
            assert 5 <= nan_rows.sum() <= 90 and not nan_rows[set_id == 1].any()
        assert np.array_equal(np.isnan(got), np.isnan(want))


def _tutorial_stations(S, ps):
    st = make_stations(DATA, S, yerr=True)
    for joint, p in zip(st, ps):
        joint.targets[1].moddata.plugin.set_modelparams(p=p)
    return st


def _fill(plan, n):
    plan.packed[:n] = 0.0
    plan.packed[:n, 0, 0], plan.packed[:n, 1, :2], plan.packed[:n, 2, :2], plan.packed[:n, 3, :2] = 30., 6., 3.5, 2.7
    plan.nlay[:n] = 2
    plan.noise[:n] = [0.0, 0.02, 0.9, 0.01]


def test_gpu_plan_rf_slowness_lifecycle_and_values():
    """bh_eval_set_rf_slowness: after the observations, once, before the first submit, nsets that of the observations,
    finite values; four rows of chains at three stations get the logL of three single-station plans."""
    from bayhunter_amd import _lib
    from bayhunter_amd.stations import observation_tables, rf_slowness_table
    ps = [5.2, 6.4, 7.9]
    st = _tutorial_stations(3, ps)
    for j in st:
        j.set_target_covariance([True, True], [0.0, 0.9], 1e-5)
    yobs, scale, logdet = observation_tables(st)
    table = rf_slowness_table(st)
    assert np.array_equal(table, [[5.2], [6.4], [7.9]])
    soc = np.array([0, 0, 1, 2], dtype=np.int32)
    with st[0].eval_plan(16, 12) as plan:
        with pytest.raises(_lib.BayHunterAmdError, match='bh_eval_set_observations first'):
            plan.set_rf_slowness(table)
        plan.set_observations(yobs, soc, scale, logdet)
        with pytest.raises(_lib.BayHunterAmdError, match=r'nsets = 2.*3 sets'):
            plan.set_rf_slowness(table[:2])
        nan = table.copy()
        nan[1, 0] = np.nan
        with pytest.raises(_lib.BayHunterAmdError, match=r'p\[1\]\[0\] is not finite'):
            plan.set_rf_slowness(nan)
        with pytest.raises(ValueError):
            plan.set_rf_slowness(np.zeros((3, 2)))
        plan.set_rf_slowness(table)
        with pytest.raises(_lib.BayHunterAmdError, match='already'):
            plan.set_rf_slowness(table)
        _fill(plan, 4)
        plan.chain[:4] = [0, 1, 2, 3]
        plan.submit(4)
        logL, mis = (a.copy() for a in plan.wait())
        with pytest.raises(_lib.BayHunterAmdError, match='after bh_eval_submit'):
            plan.set_rf_slowness(table)
    assert np.isfinite(logL).all() and logL[0] == logL[1] and len(set(logL[1:])) == 3
    for s, row in ((0, 0), (1, 2), (2, 3)):                             # the plan of that station alone, at its own p
        with st[s].eval_plan(16, 12) as one:
            _fill(one, 1)
            one.chain[:1] = 0
            one.submit(1)
            l1, m1 = one.wait()
            assert l1[0] == logL[row] and np.array_equal(m1[0], mis[row]), s
    # the same observations without the table: every row at station 0's p -- other numbers for stations 1 and 2
    with st[0].eval_plan(16, 12) as plan:
        plan.set_observations(yobs, soc, scale, logdet)
        _fill(plan, 4)
        plan.chain[:4] = [0, 1, 2, 3]
        plan.submit(4)
        shared = plan.wait()[0].copy()
    assert shared[0] == logL[0] and shared[2] != logL[2] and shared[3] != logL[3]
    with st[0].eval_plan(16, 12) as plan:
        plan.submit(0)
        with pytest.raises(_lib.BayHunterAmdError, match='after bh_eval_submit'):
            plan.set_rf_slowness(table)


def test_gpu_station_pool_with_per_station_slowness_equals_single_pools(tmp_path):
    """5 stations x 4 chains, p from 4.5 to 8.5 s/deg, two chain groups (the boundary inside station 2), look-ahead 5,
    yerr-scaled dispersion + dense Gaussian receiver-function noise: every station equals its own ChainPool exactly,
    and so do its views' datafits(), posterior() and saved files."""
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool
    case = CASES['tutorial']
    ip, priors, nmodels = dict(case['initparams'], iter_burnin=80, iter_main=40), case['priors'], 121
    ps = [4.5, 5.5, 6.5, 7.5, 8.5]
    rs = [3, 1, 4, 15, 9]
    with StationPool(_tutorial_stations(5, ps), ip, priors, chains_per_station=4, random_seeds=rs, groups=2, lookahead=5,
                     nmodels=nmodels, per_station=('p',)) as pool:
        pool.run()
    assert [(g.first, g.last) for g in pool.pool.groups] == [(0, 10), (10, 20)]
    pool.save(str(tmp_path / 'all'))
    for s, joint in enumerate(_tutorial_stations(5, ps)):
        with ChainPool(joint, ip, priors, random_seed=rs[s], nchains=4, nmodels=nmodels) as single:
            single.run()
        view = pool.station(s)
        _assert_same_chains(view, single)
        assert np.isfinite(single.likes[:, 0]).all()
        _assert_equal_trees(view.posterior(dev=0.5), single.posterior(dev=0.5), 'posterior')
        _assert_equal_trees(view.datafits(dev=0.5), single.datafits(dev=0.5), 'datafits')
        single.save(str(tmp_path / ('one%d' % s)))
        mine, ref = tmp_path / 'all' / pool.names[s] / 'data', tmp_path / ('one%d' % s) / 'data'
        files = sorted(f for f in os.listdir(str(ref)) if f.endswith('.npy'))
        assert files and files == sorted(f for f in os.listdir(str(mine)) if f.endswith('.npy'))
        for f in files:
            assert (mine / f).read_bytes() == (ref / f).read_bytes(), (s, f)


def test_gpu_same_slowness_everywhere_with_and_without_the_opt_in():
    """Stations that all have p = 6.4: the per-row form (opt-in) against the uniform form (no opt-in) through the
    whole stack -- identical chains."""
    from bayhunter_amd.stations import StationPool
    case = CASES['tutorial']
    ip, priors, nmodels = dict(case['initparams'], iter_burnin=80, iter_main=40), case['priors'], 121
    pools = []
    for per in ((), ('p',)):
        with StationPool(make_stations(DATA, 4, yerr=True), ip, priors, chains_per_station=4, random_seeds=[2, 7, 1, 8],
                         groups=2, nmodels=nmodels, per_station=per) as pool:
            pool.run()
        pools.append(pool)
    _assert_same_chains(pools[1].pool, pools[0].pool)
    assert np.isfinite(pools[0].pool.likes[:, 0]).all()
