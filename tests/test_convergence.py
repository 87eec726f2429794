"""CPU tier of the convergence diagnostics (bayhunter_amd/convergence.py, selection.half_chain_series,
csrc/autocov_core.h, csrc/autocov.hip):

* the core of the autocovariances, compiled with g++ and walked as the kernel walks it (tests/hostsim/autocov_sim.cpp),
  agrees with the numpy restatement (tests/convergence_ref.py) within tests/convergence_tolerances.py and is bit for bit
  itself under other tile lengths and lag groupings;
* half_chain_series gives the brute-force expansion of pool.weighted(i)[2] on a small host pool;
* the rules (split R-hat, Geyer's cut, tau, ESS, the verdict) give the restatement's numbers, without a device;
* bh_autocov_sets refuses bad arguments before it touches a device;
* the kernel uses no scratch, its LDS is the plan's, and its registers leave room for two waves per SIMD;
* the walk is clean under -fsanitize=address,undefined as a stand-alone program.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import convergence_ref as ref  # noqa: E402
from convergence_tolerances import check_acov  # noqa: E402

HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
SIM_SRCS = [os.path.join(HOSTSIM, 'autocov_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h)
                                                          for h in ('autocov_core.h', 'bh_common.h')]
SIM_SRCS.append(os.path.join(ROOT, 'include', 'bayhunter_amd.h'))
FMA = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in SIM_SRCS)


def load_sim():
    so = os.path.join(HOSTSIM, 'libautocov_sim.so')
    if _stale(so):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + FMA + ['-o', so, SIM_SRCS[0]],
                       check=True)
    lib = C.CDLL(so)
    lib.as_plan.restype = C.c_long
    lib.as_plan.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.as_lags_per_thread.restype = C.c_int
    lib.as_autocov_sets.restype = C.c_int
    lib.as_autocov_sets.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


@pytest.fixture(scope='module')
def asim():
    return load_sim()


def plan(asim, nlags):
    t = C.c_int(0)
    return asim.as_plan(nlags, C.byref(t)), t.value


def sim(asim, D, w, start, mean, nlags, ncols=None, tile=0, lags_per_thread=0, max_threads=0, expect=0):
    """The twin over the host matrix D (its first `ncols` columns) -> (acov, length)."""
    D = np.ascontiguousarray(D, dtype=np.float64)
    K = D.shape[1] if ncols is None else ncols
    w = None if w is None else np.ascontiguousarray(w, dtype=np.int32)
    start = np.ascontiguousarray(start, dtype=np.int64)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    S = start.size - 1
    acov = np.full((S, K, nlags), -7.)
    length = np.full(S, -1, dtype=np.int64)
    rc = asim.as_autocov_sets(D.ctypes.data, D.shape[0], D.shape[1], K, None if w is None else w.ctypes.data,
                              start.ctypes.data, S, mean.ctypes.data, nlags, acov.ctypes.data, length.ctypes.data, tile,
                              lags_per_thread, max_threads)
    assert rc == expect
    return acov, length


# ---- the twin against the restatement -------------------------------------------------------------------------

@pytest.mark.parametrize('nlags', [1, 2, 3, 64, 65, 257, 4096])
def test_twin_agrees_with_the_restatement_and_with_itself(asim, nlags):
    _, T = plan(asim, nlags)
    D, w, start, lengths = ref.series_case(T, nlags)
    assert lengths.tolist()[:7] == [0, 1, 2, 3, 63, 64, 65] and lengths[-1] == 3 * T + 5 and w[-1] == 3 * T + 5
    K = 4                                                           # the fifth column is beyond ncols: a wider stride
    mean = ref.series_means(D, w, start)[:, :K]
    want, length, absprod = ref.autocov(D, w, start, mean, nlags, ncols=K)
    got, glen = sim(asim, D, w, start, mean, nlags, ncols=K)
    assert np.array_equal(glen, lengths) and np.array_equal(length, lengths)
    worst = check_acov(got, want, lengths, absprod, 'nlags %d' % nlags)
    print('nlags %d: worst |difference| / bound %.3f' % (nlags, worst))
    for s, n in enumerate(lengths):                                 # a lag without a pair is exactly 0
        assert np.all(got[s][:, n:] == 0) and np.all(np.signbit(got[s][:, n:]) == 0)
    # neither the tile length nor the lags of a thread nor the lags of a group change a bit
    for tile, lpt, thr in ((50, 4, 64), (T + 3, 2, 128), (7, 8, 64), (3 * T, 1, 256)):
        if nlags > 300 and lpt == 1:
            continue                                                # (one lag a thread over 4096 lags: slow, no new path)
        other, _ = sim(asim, D, w, start, mean, nlags, ncols=K, tile=tile, lags_per_thread=lpt, max_threads=thr)
        assert ref.same(other, got), (tile, lpt, thr)


def test_twin_without_weights_and_with_a_nan_in_one_column(asim):
    nlags = 65
    _, T = plan(asim, nlags)
    D, _, start, lengths = ref.series_case(T, nlags, weighted=False)
    mean = ref.series_means(D, None, start)
    want, _, absprod = ref.autocov(D, None, start, mean, nlags)
    got, glen = sim(asim, D, None, start, mean, nlags)
    assert np.array_equal(glen, lengths)
    check_acov(got, want, lengths, absprod, 'unweighted')
    # a NaN in column 2 of the longest series, far from both ends: with the others' mean handed in, exactly the lags
    # whose chain reads it are NaN (here all 65), and no other column or series moves a bit
    D2 = D.copy()
    s = len(lengths) - 1
    D2[start[s] + 1000, 2] = np.nan
    want2, _, absprod2 = ref.autocov(D2, None, start, mean, nlags)
    got2, _ = sim(asim, D2, None, start, mean, nlags)
    assert np.isnan(got2[s, 2]).all() and np.isnan(want2[s, 2]).all()
    keep = np.ones(got.shape, dtype=bool)
    keep[s, 2] = False
    assert ref.same(got2[keep], got[keep])
    # in the middle of the series of three samples only lags 0 and 1 read it: the definition, not a blanket rule
    D3 = D.copy()
    assert lengths[3] == 3
    D3[start[3] + 1, 2] = np.nan
    got3, _ = sim(asim, D3, None, start, mean, nlags)
    want3, _, absprod3 = ref.autocov(D3, None, start, mean, nlags)
    check_acov(got3, want3, lengths, absprod3, 'NaN in the middle of three')
    assert np.isnan(got3[3, 2, :2]).all() and np.isfinite(got3[3, 2, 2]) and got3[3, 2, 2] != 0
    assert sim(asim, D, np.where(np.arange(D.shape[0]) == 5, -1, 1), start, mean, nlags, expect=1)


def test_the_lds_plan(asim):
    from bayhunter_amd import _lib
    for nlags in (1, 64, 1024, _lib.AUTOCOV_MAX_LAGS):
        bytes_, T = plan(asim, nlags)
        assert T >= 1024 and 8 * (T + nlags) <= bytes_ <= 8 * (T + nlags + 8) and bytes_ <= 64 * 1024


# ---- which rows -------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def station_pool(oracle):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES, oracle_evaluator
    from station_scenario import make_stations, station_evaluator
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=90, iter_main=60)
    stations = make_stations(os.path.join(GOLDEN, 'tutorial_observed'), 3, oracle=oracle, yerr=True)
    ev = station_evaluator([oracle_evaluator(j) for j in stations])
    return StationPool(stations, ip, case['priors'], chains_per_station=4, random_seeds=[7, 8, 9], evaluator=ev,
                       nmodels=151).run()


def brute_force(view, chains):
    """The half chains of `chains` of a view from the expanded main phase of weighted(): [(chain, half, likes, vpvs)]."""
    first = {}
    full = {}
    for i in chains:
        it = view.chain(i)['iter']
        first[i] = int(it[it >= 0][0])
        full[i] = view.weighted(i)[2]
        assert full[i][1].size == view.iter_main - first[i]
    t0 = max(first.values())
    n = (view.iter_main - t0) // 2
    out = []
    for i in chains:
        for lo, hi in ((view.iter_main - 2 * n, view.iter_main - n), (view.iter_main - n, view.iter_main)):
            out.append((i, full[i][1][lo - first[i]:hi - first[i]], full[i][4][lo - first[i]:hi - first[i]]))
    return n, t0, first, out


def check_against_brute_force(station_pool, dev, exclude):
    """-> (rows in both halves of their chain, stations whose window a late chain shortened, chains left out)"""
    from bayhunter_amd.selection import half_chain_series, pool_rows
    pool, c = station_pool, station_pool.chains_per_station
    hs = half_chain_series(pool.pool, c, dev, exclude)
    assert not hs['failed'] and hs['group_start'][0] == 0 and hs['group_start'][-1] == hs['series_start'].size - 1
    both = dropped = late = 0
    for s in range(3):
        view = pool.station(s)
        chains = np.unique(pool_rows(view, 'weighted', dev, exclude)[0])
        dropped += c - chains.size
        n, t0, first, want = brute_force(view, chains)
        late += len(set(first.values())) > 1 and t0 > min(first.values())
        a, b = hs['group_start'][s], hs['group_start'][s + 1]
        assert b - a == 2 * chains.size and hs['n'][s] == n and tuple(hs['window'][s]) == (view.iter_main - 2 * n, view.iter_main)
        assert np.array_equal(hs['chains'][a // 2:b // 2] - s * c, chains)
        assert np.array_equal(hs['first_iter'][s * c + chains], [first[i] for i in chains])
        for j, (i, likes, vpvs) in enumerate(want):
            lo, hi = hs['series_start'][a + j], hs['series_start'][a + j + 1]
            ci, ri, w = hs['ci'][lo:hi], hs['ri'][lo:hi], hs['w'][lo:hi]
            assert np.all(ci == s * c + i) and np.all(w > 0) and w.sum() == n and np.all(np.diff(ri) > 0)
            assert np.array_equal(np.repeat(pool.pool.likes[ci, ri], w), likes)
            assert np.array_equal(np.repeat(pool.pool.vpvs[ci, ri], w), vpvs)
            if j % 2:                                               # a row that straddles the boundary is in both halves
                plo = hs['series_start'][a + j - 1]
                both += hs['ri'][lo] == hs['ri'][lo - 1] and plo < lo
        # the one-group form on the view: the same entries
        one = half_chain_series(view, c, dev, exclude)
        lo, hi = hs['series_start'][a], hs['series_start'][b]
        assert np.array_equal(one['ci'], hs['ci'][lo:hi] - s * c) and np.array_equal(one['ri'], hs['ri'][lo:hi])
        assert np.array_equal(one['w'], hs['w'][lo:hi]) and np.array_equal(one['series_start'], hs['series_start'][a:b + 1] - lo)
    return both, late, dropped


@pytest.mark.parametrize('dev,exclude', [(0.05, True), (0.0005, True), (0.05, False)])
def test_half_chain_series_is_the_brute_force_expansion(station_pool, dev, exclude):
    both, _, dropped = check_against_brute_force(station_pool, dev, exclude)
    assert both > 0                                                 # rows that straddle the boundary of the halves
    assert exclude is False or dev > 0.001 or dropped > 0           # the tight bound does leave an outlier chain out


def test_a_late_first_acceptance_shortens_the_stations_window(station_pool):
    from bayhunter_amd.selection import half_chain_series
    inner, c = station_pool.pool, station_pool.chains_per_station
    before = half_chain_series(inner, c, 0.05, False)
    keep = inner.iter.copy()
    try:
        it = inner.iter[c + 2]                                      # chain 2 of station 1
        early = (it >= 0) & (it < 11)
        assert early.any()
        it[it < 0] -= 11                                            # counted to the burn-in: the main phase begins late
        it[early] -= 11
        both, late, _ = check_against_brute_force(station_pool, 0.05, False)
        after = half_chain_series(inner, c, 0.05, False)
    finally:
        inner.iter[:] = keep
    assert late >= 1 and both > 0
    assert after['first_iter'][c + 2] >= 11 > before['first_iter'][c + 2]
    assert after['n'][1] < before['n'][1] and after['window'][1][0] >= 11 and after['n'][0] == before['n'][0]


def test_a_station_with_a_short_window_is_failed(station_pool):
    """A chain whose first main-phase acceptance comes 5 iterations before the end leaves its station n = 2 < 4."""
    from bayhunter_amd.selection import half_chain_series
    inner, c = station_pool.pool, station_pool.chains_per_station
    keep = inner.iter.copy()
    try:
        ch = 2 * c + 1
        it = inner.iter[ch]
        early = (it >= 0) & (it < inner.iter_main - 5)
        assert early.any()
        it[it < 0] -= inner.iter_main - 5                           # counted to the burn-in: the main phase begins late
        it[early] -= inner.iter_main - 5
        hs = half_chain_series(inner, c, 0.05, False)
        assert list(hs['failed']) == [2] and 'window' in hs['failed'][2]
        assert hs['group_start'][2] == hs['group_start'][3] and tuple(hs['window'][2]) == (-1, -1) and hs['n'][2] == 0
        assert np.all(hs['ci'] < 2 * c) and hs['n'][0] >= 4
    finally:
        inner.iter[:] = keep


# ---- the rules ----------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def ar1(asim):
    """The four AR(1) sets with the restatement's means and autocovariances and the twin's."""
    out = []
    for name, D, w, start, n, nlags in ref.ar1_sets():
        mean = ref.series_means(D, w, start)
        want, length, absprod = ref.autocov(D, w, start, mean, nlags)
        assert np.all(length == n) and start.size == 9
        got, _ = sim(asim, D, w, start, mean, nlags)
        check_acov(got, want, length, absprod, name)
        out.append(dict(name=name, D=D, w=w, start=start, n=n, nlags=nlags, mean=mean, acov=want, twin=got))
    return out


def test_the_rules_on_four_ar1_sets(ar1):
    from bayhunter_amd import convergence as cv
    tau_of = {}
    for case in ar1:
        n, mean = case['n'], case['mean'][:, 0]
        want = ref.diagnose(mean, case['acov'][:, 0], n)
        got = cv.diagnose(mean, case['acov'][:, 0], n)
        print(case['name'], 'n', n, 'cut', want['cut'], 'of', min(case['nlags'], n) // 2, 'tau', want['tau'], 'rhat',
              want['rhat'], 'ess', want['ess'])
        for k in ('rhat', 'tau', 'ess', 'W', 'B', 'var_plus', 'mean'):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-13, atol=0, err_msg=k)
        assert got['truncated'] == want['truncated'] and not got['constant']
        kept = want['rho'].size
        np.testing.assert_allclose(got['acf'][:kept], want['rho'], rtol=0, atol=1e-13)
        assert np.isnan(got['acf'][kept:]).all() and got['acf'].size == case['nlags']
        assert 0.9 < got['rhat'] < 2. and got['ess'] == pytest.approx(8 * n / got['tau'])
        tau_of[case['name']] = got['tau']
        # Every outcome by reasoning, none from a run.  With N = 8 n samples and integrated time tau the estimated
        # autocorrelations scatter by about sqrt(tau / N) around rho_k + (var+ - W) / var+, the latter about tau / n.
        pairs = min(case['nlags'], n) // 2
        lo, hi = {
            # rho_k = 0.8^(k / 2.5) (a value is held 2.5 iterations on average), tau about 22, scatter of a pair 0.1:
            # pairs 0 .. 2 (lags < 6, 2 rho > 1.1) stand 10 sigma above 0; beyond lag 100 rho < 1e-4 and the 200 pairs
            # left are noise around 0.04, in stretches of about 11 pairs: none of 18 stretches dipping has 0.65^18 < 1e-3
            'phi 0.8': (3, pairs),
            # rho_k = 0.5^k, tau 3, scatter of a pair 0.03: pairs 0 and 1 (1.5, 0.375) are sure; beyond lag 24 the
            # 20 pairs left are noise around 0.006, nearly independent: 0.58^20 = 2e-5
            'phi 0.5': (2, pairs),
            # P_0 = 1 + rho_1 is sure; every later pair is negative with probability 1/2: 2^-40 for 40 in a row
            'white': (1, 41),
            # rho_16 = 0.95^8 = 0.66 with scatter 0.13 (tau about 80, N = 4700): every pair above 1.3, 5 sigma of 0.26
            'phi 0.95 short': (None, None)}[case['name']]
        if lo is None:
            assert want['truncated'] and want['cut'] is None
        else:
            assert not want['truncated'] and lo <= want['cut'] < hi, (case['name'], want['cut'])
        # per chain: the same from its own two halves
        grp = cv.group_diagnostics(case['mean'], case['acov'], n, ['x'])['x']
        for i in range(4):
            one = ref.diagnose(mean[2 * i:2 * i + 2], case['acov'][2 * i:2 * i + 2, 0], n)
            np.testing.assert_allclose([grp['tau_chain'][i], grp['ess_chain'][i]], [one['tau'], one['ess']], rtol=1e-13)
        assert grp['rhat'] == got['rhat'] and grp['tau'] == got['tau']
    # white noise: tau = 1 + 2 rho_1 + 2 (the kept later pairs).  sd(rho_1) = 1 / sqrt(M n) = 1 / 40, so 2 rho_1 stays
    # within 5 sigma = 0.25; a kept pair P_k >= 0 has sd sqrt(2) / 40 and adds 2 P_k <= 10 sigma = 0.36
    white = next(c for c in ar1 if c['name'] == 'white')
    assert 8 * white['n'] == 1600
    cut = ref.diagnose(white['mean'][:, 0], white['acov'][:, 0], white['n'])['cut']
    assert abs(tau_of['white'] - 1.) <= 0.25 + 0.36 * (cut - 1)
    # an AR(1) value held w iterations on average is slower than its (1 + phi) / (1 - phi)
    assert tau_of['phi 0.8'] > 9. and tau_of['phi 0.5'] > 2.
    assert tau_of['phi 0.95 short'] < 2 * 16                         # at most 2 per lag kept: the lower bound it is


def test_constant_negative_first_pair_unequal_lengths_and_the_verdict():
    from bayhunter_amd import convergence as cv
    n, K = 100, 8
    const = cv.diagnose(np.full(4, 3.5), np.zeros((4, K)), n)
    assert const['constant'] and const['W'] == 0 and const['mean'] == 3.5
    assert all(np.isnan(const[k]) for k in ('rhat', 'tau', 'ess')) and np.isnan(const['acf']).all()
    assert not cv.converged(const, 2)
    # an alternating series: rho_1 close to -1, so P_0 < 0
    acov = np.tile(np.array([1., -0.99, 0.98, -0.97, 0.96, -0.95, 0.94, -0.93]) * 0.5, (4, 1))
    neg = cv.diagnose(np.zeros(4), acov, n)
    want = ref.diagnose(np.zeros(4), acov, n)
    assert want['cut'] == 0 and np.isnan(want['tau'])
    assert np.isnan(neg['tau']) and np.isnan(neg['ess']) and not neg['truncated'] and neg['rhat'] == want['rhat']
    assert not cv.converged(neg, 2)
    with pytest.raises(ValueError):
        cv.group_diagnostics(np.zeros((3, 1)), np.zeros((3, 1, K)), n, ['x'])
    with pytest.raises(ValueError):
        cv.diagnose(np.zeros(3), np.zeros((4, K)), n)
    good = dict(rhat=1.005, ess=450., truncated=False)
    assert cv.converged(good, 4) and not cv.converged(good, 5)       # 100 per chain
    assert cv.converged(good, 5, ess_min=400.) and not cv.converged(good, 4, rhat_max=1.001)
    assert not cv.converged(dict(good, truncated=True), 4) and not cv.converged(dict(good, rhat=np.nan), 4)
    assert cv.geyer([1., 0.5, 0.2, 0.1]) == (pytest.approx(-1 + 2 * 1.8), 2, True)
    assert cv.geyer([1., 0.5, -0.2, 0.1, 0.3, 0.3])[:2] == (pytest.approx(2.), 1)
    tau, kept, trunc = cv.geyer([1., 0.2, 0.6, 0.8, -1., 0.])        # made non-increasing: 1.2, min(1.4, 1.2)
    assert (tau, kept, trunc) == (pytest.approx(-1 + 2 * 2.4), 2, False)


def test_vs_at_a_depth():
    from bayhunter_amd import convergence as cv
    from bayhunter_amd.posterior import stepmodel
    nan = np.nan
    rows = np.array([[3.0, 3.6, 4.4, 2., 21., 40., nan, nan],       # vs | z of the nuclei: interfaces at 11.5 and 30.5
                     [3.2, 4.5, 5., 55., nan, nan, nan, nan],       # one interface at 30
                     [3.9, 9., nan, nan, nan, nan, nan, nan]])      # a half space
    got = cv.vs_at(rows, (5., 30., 11.5, 30.5, 200.))
    assert got.tolist() == [[3.0, 3.6, 3.6, 4.4, 4.4], [3.2, 4.5, 3.2, 4.5, 4.5], [3.9] * 5]
    for r, row in enumerate(rows):                                   # posterior.stepmodel's layering, strictly inside a layer
        vs, dep = stepmodel(row)
        for j, z in enumerate((5., 30.2, 11.4, 30.7, 140.)):
            i = np.searchsorted(dep[1::2], z, side='right')
            assert cv.vs_at(rows[r:r + 1], (z,))[0, 0] == vs[2 * min(i, vs.size // 2 - 1)], (r, z)


# ---- the library ------------------------------------------------------------------------------------------

def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    nodev = C.c_void_p(16)                  # never dereferenced: the arguments are checked first
    mean, acov, length = np.zeros((2, 5)), np.zeros((2, 5, 8)), np.zeros(2, dtype=np.int64)

    def call(D=nodev, nrows=10, stride=5, ncols=5, start=(0, 4, 10), nseries=2, mean=mean, nlags=8, acov=acov,
             length=length):
        st = None if start is None else np.asarray(start, dtype=np.int64)
        return lib.bh_autocov_sets(D, nrows, stride, ncols, None, None if st is None else st.ctypes.data, nseries,
                                   None if mean is None else mean.ctypes.data, nlags,
                                   None if acov is None else acov.ctypes.data,
                                   None if length is None else length.ctypes.data, None)
    err = lambda: lib.bh_last_error()
    assert call(D=None) == E and call(nrows=0, start=(0, 0, 0)) == E and b'empty' in err()
    assert call(nrows=(1 << 32) + 1, start=(0, 4, (1 << 32) + 1)) == E and b'2^32' in err()
    assert call(stride=4) == E and b'stride' in err() and call(ncols=0) == E
    assert call(nseries=0) == E and b'series' in err()
    assert call(start=None) == E
    assert call(start=(0, 6, 4, 10), nseries=3) == E and b'ascending' in err()
    assert call(start=(0, 4, 9)) == E and b'end at nrows' in err() and call(start=(1, 4, 10)) == E
    assert call(nlags=0) == E and b'lags' in err() and call(nlags=_lib.AUTOCOV_MAX_LAGS + 1) == E and b'lags' in err()
    assert call(mean=None) == E and call(acov=None) == E and call(length=None) == E and b'mean, acov and length' in err()
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read()
    assert '#define BH_AUTOCOV_MAX_LAGS %d' % _lib.AUTOCOV_MAX_LAGS in header and 'int  bh_autocov_sets(' in header
    assert 'autocov.hip' in _lib.SOURCES and 'autocov_core.h' in _lib.HEADERS


def test_python_layer_refuses_bad_arguments():
    from bayhunter_amd import convergence as cv, scalars
    cols = scalars.Columns(np.zeros((10, 2)), ['f8', 'f8'])
    with pytest.raises(ValueError, match='set_start'):
        cv.summarize(cols, None, [0, 6, 4, 10], [0, 3], device='cpu')
    with pytest.raises(ValueError, match='set_start'):
        cv.summarize(cols, None, [0, 5, 10], [0, 1], device='cpu')
    with pytest.raises(ValueError, match='nlags'):
        cv.summarize(cols, None, [0, 5, 10], [0, 2], nlags=4097, device='cpu')
    with pytest.raises(ValueError, match='one weight per row'):
        cv.summarize(cols, np.ones(9, dtype=np.int32), [0, 5, 10], [0, 2], device='cpu')
    with pytest.raises(ValueError, match='Columns'):
        cv.summarize(np.zeros((10, 2)), None, [0, 5, 10], [0, 2], device='cpu')


def test_autocov_kernel_resources(asim):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    from bayhunter_amd import _lib
    r = kernel_resources('autocov.hip')
    mine = {k: v for k, v in r.items() if 'autocov_kernel' in k}
    assert len(mine) == 1, sorted(r)
    assert all(v['scratch'] == 0 for v in r.values()), r
    L = asim.as_lags_per_thread()
    for nlags in (1024, _lib.AUTOCOV_MAX_LAGS):
        dyn, T = plan(asim, nlags)
        assert dyn == 8 * L * -(-(T + nlags) // L), (nlags, dyn)        # L planes of ceil((T + nlags) / L) doubles
        for k, v in mine.items():
            assert v['lds'] == 0, (k, v)                                # no static part: the launch's LDS is the plan
            assert v['lds'] + dyn <= 64 * 1024, (k, v, dyn)             # (a CU has 160 KiB: two workgroups at least)
    for k, v in mine.items():
        # next_free_vgpr counts the unified file, accumulation registers included: 512 per SIMD lane, two waves at 256
        assert v['vgpr'] <= 256, (k, v)


def test_the_walk_is_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main) over the CPU tier's shapes, built with -fsanitize=address,undefined."""
    exe = str(tmp_path / 'autocov_san')
    build = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=undefined', '-DAUTOCOV_SIM_MAIN'] + FMA + ['-o', exe, SIM_SRCS[0]],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and 'results equal' in run.stdout, (run.stdout[-400:], run.stderr[-2000:])
