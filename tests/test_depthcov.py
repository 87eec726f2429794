"""CPU tier of the depth-to-depth covariance (bayhunter_amd/covariance.py, csrc/depthcov_core.h, csrc/depthcov.hip):

* the restatement (tests/depthcov_ref.py) is np.cov on a matrix that really is expanded;
* the host twin (tests/hostsim/depthcov_sim.cpp: the core compiled with g++, the kernel's blocking, one fma chain per
  cell) agrees with the restatement within tests/depthcov_tolerances.py, is exactly symmetric, and gives a set the same
  bits alone, at another offset and among other sets;
* the host formulas of covariance.py: (S - r1 r1^T / W) / W, NaN correlation at zero variance, a centre moved by 1e-3;
* bh_depthcov_sets and the Python layer refuse bad arguments before they touch a device;
* the kernel uses no scratch, its LDS fits a CU and its registers leave room for two waves per SIMD.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import depthcov_ref as ref  # noqa: E402
import depthcov_tolerances as tol  # noqa: E402

HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
SIM_SRCS = [os.path.join(HOSTSIM, 'depthcov_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                           ('depthcov_core.h', 'posterior_core.h', 'stats_core.h',
                                                            'bh_common.h')]
SIM_SRCS.append(os.path.join(ROOT, 'include', 'bayhunter_amd.h'))
FMA = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []


def load_sim():
    so = os.path.join(HOSTSIM, 'libdepthcov_sim.so')
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SIM_SRCS):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + FMA + ['-o', so, SIM_SRCS[0]],
                       check=True)
    lib = C.CDLL(so)
    lib.ds_depthcov_sets.restype = C.c_int
    lib.ds_depthcov_sets.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.ds_pair.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return lib


@pytest.fixture(scope='module')
def dsim():
    return load_sim()


def sim(dsim, rows, weights, extra, set_start, dep, center, block_rows=0, expect=0):
    """The twin over host arrays -> (S, r1, total)."""
    rows = np.ascontiguousarray(rows)
    assert rows.dtype in (np.float32, np.float64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
    extra = None if extra is None else np.ascontiguousarray(extra, dtype=np.float64)
    set_start = np.ascontiguousarray(set_start, dtype=np.int64)
    dep, center = np.ascontiguousarray(dep, dtype=np.float64), np.ascontiguousarray(center, dtype=np.float64)
    Z, nextra = set_start.size - 1, 0 if extra is None else extra.shape[1]
    K = dep.size + nextra
    S, r1, total = np.full((Z, K, K), -7.), np.full((Z, K), -7.), np.full(Z, -1, dtype=np.int64)
    rc = dsim.ds_depthcov_sets(rows.ctypes.data, int(rows.dtype == np.float64), rows.shape[0], rows.shape[1], rows.shape[1],
                               None if w is None else w.ctypes.data, None if extra is None else extra.ctypes.data,
                               nextra, nextra, set_start.ctypes.data, Z, dep.ctypes.data, dep.size, center.ctypes.data,
                               S.ctypes.data, r1.ctypes.data, total.ctypes.data, block_rows)
    assert rc == expect
    return S, r1, total


def sim_case(dsim, c, **kw):
    return sim(dsim, c['rows'], c['weights'], c['extra'], c['set_start'], c['dep'], c['center'], **kw)


# ---- the restatement ---------------------------------------------------------------------------------------------

def test_restatement_is_numpy_cov_of_the_expanded_matrix():
    rng = np.random.default_rng(5)
    rows = ref.random_rows(rng, 60, np.float32)
    rows[7] = np.nan
    w = rng.integers(0, 6, size=60)
    extra = rng.uniform(1.6, 1.9, size=(60, 2))
    dep = np.asarray([0., 3., 10., 25., 61.])
    X, has = ref.columns(rows, dep, extra)
    keep = (w > 0) & has
    expanded = np.repeat(X[keep], w[keep], axis=0)                   # the matrix the weights stand for
    assert expanded.shape == (w[keep].sum(), 7)
    want_cov, want_corr = np.cov(expanded.T, bias=True), np.corrcoef(expanded.T)
    for center in (expanded.mean(axis=0), expanded.mean(axis=0) + 1e-3, np.zeros(7)):
        m = ref.moments(rows, w, extra, [0, 60], dep, center[None, :])
        assert m['total'][0] == expanded.shape[0] and m['terms'][0] == keep.sum()
        cov, corr = ref.cov_corr(m['S'][0], m['r1'][0], m['total'][0])
        scale = np.sqrt(np.outer(np.diag(want_cov), np.diag(want_cov)))
        assert np.all(np.abs(cov.astype(np.float64) - want_cov) <= 1e-12 * (scale + np.outer(center, center) ** 2))
        assert np.allclose(corr.astype(np.float64), want_corr, rtol=0, atol=1e-9)


# ---- the twin ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fp64', [False, True])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('ndep,nextra', [(2, 0), (16, 0), (17, 1), (33, 3), (2, 1), (16, 3)])
def test_twin_agrees_with_the_restatement(dsim, ndep, nextra, fp64, weighted):
    B = dsim.ds_block_rows()
    from bayhunter_amd import _lib
    assert B == _lib.DEPTHCOV_BLOCK_ROWS and dsim.ds_max_k() == _lib.DEPTHCOV_MAX_K
    c = ref.case(B, ndep, nextra, fp64, weighted)
    want = ref.moments(c['rows'], c['weights'], c['extra'], c['set_start'], c['dep'], c['center'])
    assert want['total'][2] == 0 and want['total'][5] == 0 and np.all(want['total'][[0, 1, 3, 4, 6, 7]] > 0)
    S, r1, total = sim_case(dsim, c)
    worst = tol.check_moments(S, r1, total, want, 'ndep %d nextra %d' % (ndep, nextra))
    print('ndep %d nextra %d fp64 %d weighted %d: worst |difference| / bound %.3g' % (ndep, nextra, fp64, weighted, worst))
    assert np.array_equal(S, np.swapaxes(S, 1, 2))                    # exactly symmetric


def test_twin_set_independence(dsim):
    """A set alone, at another offset in rows, gives the bits it has in the joint call; two runs agree."""
    B = dsim.ds_block_rows()
    c = ref.case(B, 17, 1, False, True)
    S, r1, total = sim_case(dsim, c)
    S2, r12, total2 = sim_case(dsim, c)
    assert S.tobytes() == S2.tobytes() and r1.tobytes() == r12.tobytes() and np.array_equal(total, total2)
    st = c['set_start']
    for z in range(len(st) - 1):
        a, b = int(st[z]), int(st[z + 1])
        if a == b:
            continue
        pad = 3                                                       # three other rows before the set, in a set of their own
        sl = lambda x: None if x is None else np.concatenate((x[:pad], x[a:b]))
        Sz, rz, tz = sim(dsim, sl(c['rows']), sl(c['weights']), sl(c['extra']), [0, pad, pad + b - a], c['dep'],
                         np.stack((c['center'][0], c['center'][z])))
        assert Sz[1].tobytes() == S[z].tobytes() and rz[1].tobytes() == r1[z].tobytes() and tz[1] == total[z], z


def test_twin_blocks_add_up_in_order(dsim):
    """With blocks of 4 rows the result is the fold of the 4-row partials in ascending order, from 0.0."""
    rng = np.random.default_rng(11)
    rows = ref.random_rows(rng, 11, np.float64)
    w = rng.integers(1, 9, size=11).astype(np.int32)
    dep = np.asarray([1., 20., 45.])
    center = ref.weighted_means(rows, w, None, [0, 11], dep)
    S, r1, total = sim(dsim, rows, w, None, [0, 11], dep, center, block_rows=4)
    acc, racc = np.zeros((3, 3)), np.zeros(3)
    for a in range(0, 11, 4):
        Sb, rb, _ = sim(dsim, rows[a:a + 4], w[a:a + 4], None, [0, min(4, 11 - a)], dep, center, block_rows=4)
        acc, racc = acc + Sb[0], racc + rb[0]
    assert S[0].tobytes() == acc.tobytes() and r1[0].tobytes() == racc.tobytes() and total[0] == w.sum()


def test_tile_pairs_and_accumulator_slots(dsim):
    """The pairs enumerate the upper triangle row by row; the accumulator slot is the MFMA's layout: the column on the
    lane's low four bits, row = (lane >> 4) + 4 reg."""
    for T in (1, 2, 3, 13, 16):
        seen = []
        for p in range(T * (T + 1) // 2):
            i, j = C.c_int(-1), C.c_int(-1)
            dsim.ds_pair(T, p, C.byref(i), C.byref(j))
            seen.append((i.value, j.value))
        assert seen == [(i, j) for i in range(T) for j in range(i, T)]
    slots = set()
    for m in range(16):
        for n in range(16):
            s = dsim.ds_acc_slot(m, n)
            reg, lane = s // 64, s % 64
            assert lane & 15 == n and (lane >> 4) + 4 * reg == m
            slots.add(s)
    assert slots == set(range(256))
    assert dsim.ds_npairs(204) == 91 and dsim.ds_group_pairs() >= 91   # 201 depths and three extras: one group of pairs


# ---- the host formulas ------------------------------------------------------------------------------------------------

def test_from_moments_is_the_restatements_covariance(dsim):
    from bayhunter_amd import covariance as cv
    B = dsim.ds_block_rows()
    c = ref.case(B, 17, 1, True, True)
    want = ref.moments(c['rows'], c['weights'], c['extra'], c['set_start'], c['dep'], c['center'])
    S, r1, total = sim_case(dsim, c)
    moved = c['center'] + 1e-3
    want_m = ref.moments(c['rows'], c['weights'], c['extra'], c['set_start'], c['dep'], moved)
    Sm, r1m, totalm = sim(dsim, c['rows'], c['weights'], c['extra'], c['set_start'], c['dep'], moved)
    tol.check_moments(Sm, r1m, totalm, want_m, 'moved centre')
    for z in np.nonzero(total > 0)[0]:
        cov, corr, std = cv.from_moments(S[z], r1[z], total[z])
        wcov, wcorr = ref.cov_corr(want['S'][z], want['r1'][z], want['total'][z])
        assert np.all(np.abs(cov - wcov) <= tol.cov_bound(want, z)), z
        assert np.array_equal(std, np.sqrt(np.diagonal(cov)))
        # the centre moved by 1e-3: the same covariance, to the bound of both (not bit for bit)
        covm, _, _ = cv.from_moments(Sm[z], r1m[z], totalm[z])
        both = tol.cov_bound(want, z, recentred=True) + tol.cov_bound(want_m, z, recentred=True)
        assert np.all(np.abs(covm.astype(np.longdouble) - cov) <= both), (z, np.abs(covm - cov).max(), both.max())
    with pytest.raises(ValueError):
        cv.from_moments(np.zeros((2, 2)), np.zeros(2), 0)
    with pytest.raises(ValueError):
        cv.from_moments(np.zeros((2, 3)), np.zeros(2), 5)


def test_from_moments_zero_variance_and_names():
    from bayhunter_amd import covariance as cv
    rng = np.random.default_rng(3)
    X = rng.normal(size=(50, 4))
    X[:, 2] = 3.5                                                     # a column of one value
    w = rng.integers(1, 5, size=50).astype(np.float64)
    c = np.asarray([0.1, -0.2, 3.5, 0.])
    d = X - c
    cov, corr, std = cv.from_moments((w[:, None] * d).T @ d, (w[:, None] * d).sum(axis=0), w.sum())
    assert std[2] == 0 and not np.any(cov[2]) and not np.any(cov[:, 2])
    assert np.all(np.isnan(corr[2])) and np.all(np.isnan(corr[:, 2]))
    live = [0, 1, 3]
    assert np.all(np.diagonal(corr)[live] == 1.) and np.all(np.isfinite(corr[np.ix_(live, live)]))
    expanded = np.repeat(X, w.astype(int), axis=0)
    assert np.allclose(cov, np.cov(expanded.T, bias=True), rtol=0, atol=1e-13)
    assert np.allclose(corr[np.ix_(live, live)], np.corrcoef(expanded[:, live].T), rtol=0, atol=1e-12)
    # a centre off the constant column's value by a rounding: `constant` (the scan's min == max) holds the variance at 0
    c2 = c + np.asarray([0., 0., 4.4e-16, 0.])
    d2 = X - c2
    cov2, corr2, std2 = cv.from_moments((w[:, None] * d2).T @ d2, (w[:, None] * d2).sum(axis=0), w.sum(),
                                        constant=[False, False, True, False])
    assert std2[2] == 0 and not np.any(cov2[2]) and np.all(np.isnan(corr2[2])) and np.all(np.isnan(corr2[:, 2]))
    assert cv.column_names([0., 0.5, 12.], ('vpvs',)) == ['vs@0', 'vs@0.5', 'vs@12', 'vpvs']


# ---- the library ------------------------------------------------------------------------------------------

def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    nodev = C.c_void_p(16)                  # never dereferenced: the arguments are checked first
    dep0, center, S, r1 = np.asarray([0., 1., 2.]), np.zeros((2, 4)), np.zeros((2, 4, 4)), np.zeros((2, 4))
    total = np.zeros(2, dtype=np.int64)

    def call(rows=nodev, nrows=10, stride=12, width=12, extra=nodev, extra_stride=1, nextra=1, start=(0, 4, 10), nsets=2,
             dep=dep0, ndep=3, center=center, S=S, r1=r1, total=total):
        st = None if start is None else np.asarray(start, dtype=np.int64)
        p = lambda a: None if a is None else a.ctypes.data
        return lib.bh_depthcov_sets(rows, 0, nrows, stride, width, None, extra, extra_stride, nextra, p(st), nsets, p(dep),
                                    ndep, p(center), p(S), p(r1), p(total), None)
    err = lambda: lib.bh_last_error()
    assert call(rows=None) == E and call(nrows=0, start=(0, 0, 0)) == E and b'empty' in err()
    assert call(nrows=(1 << 32) + 1, start=(0, 4, (1 << 32) + 1)) == E and b'2^32' in err()
    assert call(stride=11) == E and b'stride' in err() and call(width=1) == E
    assert call(ndep=0) == E and b'ndep' in err() and call(dep=None) == E
    assert call(dep=np.asarray([0., 2., 1.])) == E and b'ascending' in err()
    assert call(dep=np.asarray([0., 1., 1.])) == E and call(dep=np.asarray([0., np.nan, 1.])) == E
    assert call(nextra=-1) == E and call(extra=None) == E and b'extra' in err() and call(extra_stride=0) == E
    big = np.arange(_lib.DEPTHCOV_MAX_K, dtype=np.float64)
    assert call(dep=big, ndep=big.size) == E and b'above 256' in err()       # K = 256 depths + 1 extra
    assert call(nsets=0) == E and b'one set' in err()
    assert call(start=None) == E
    assert call(start=(0, 6, 4, 10), nsets=3) == E and b'ascending' in err()
    assert call(start=(0, 4, 9)) == E and b'end at nrows' in err() and call(start=(1, 4, 10)) == E
    assert call(center=None) == E and call(S=None) == E and call(r1=None) == E and call(total=None) == E
    assert b'center, S, r1 and total' in err()
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read()
    assert '#define BH_DEPTHCOV_MAX_K      %d' % _lib.DEPTHCOV_MAX_K in header
    assert '#define BH_DEPTHCOV_BLOCK_ROWS %d' % _lib.DEPTHCOV_BLOCK_ROWS in header and 'int  bh_depthcov_sets(' in header
    assert 'depthcov.hip' in _lib.SOURCES and 'depthcov_core.h' in _lib.HEADERS


def test_python_layer_refuses_bad_arguments():
    from bayhunter_amd import covariance as cv
    models = np.zeros((10, 12), dtype=np.float32)
    with pytest.raises(ValueError, match='set_start'):
        cv.summarize_sets(models, [0, 6, 4, 10], device='cpu')
    with pytest.raises(ValueError, match='dep_int'):
        cv.summarize(models, dep_int=[0., 2., 1.], device='cpu')
    with pytest.raises(ValueError, match='dep_int'):
        cv.summarize(models, dep_int=[], device='cpu')
    with pytest.raises(ValueError, match='extra'):
        cv.summarize(models, extra=np.zeros((9, 1)), extra_names=('a',), device='cpu')
    with pytest.raises(ValueError, match='extra_names'):
        cv.summarize(models, extra=np.zeros((10, 2)), extra_names=('a',), device='cpu')
    with pytest.raises(ValueError, match='at most'):
        cv.summarize(models, dep_int=np.arange(256.), extra=np.zeros((10, 1)), extra_names=('a',), device='cpu')
    with pytest.raises(ValueError, match='one weight per row'):
        cv.summarize(models, weights=np.ones(9, dtype=np.int32), device='cpu')
    with pytest.raises(ValueError, match='budget_bytes'):
        cv.summarize_sets(models, [0, 10], budget_bytes=0, device='cpu')
    with pytest.raises(ValueError, match='empty selection'):
        cv.summarize(models[:0], device='cpu')
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool, StationView
    assert callable(ChainPool.depth_covariance) and callable(StationPool.depth_covariance)
    assert StationView.depth_covariance is ChainPool.depth_covariance and 'depth_covariance()' in StationView.__doc__


def test_depthcov_kernel_resources(dsim):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    from bayhunter_amd import _lib
    r = kernel_resources('depthcov.hip')
    mine = {k: v for k, v in r.items() if 'depthcov_kernel' in k}
    assert len(mine) == 2, sorted(r)                                   # float32 and float64 rows
    assert all(v['scratch'] == 0 for v in r.values()), r
    # two stages of d and e, 16 rows each at a pitch of K padded to 16 (and off the 32-bank stride), the grid, the centre
    assert dsim.ds_lds_bytes(204) == 8 * (4 * 16 * 208 + 2 * 208)
    assert dsim.ds_lds_bytes(_lib.DEPTHCOV_MAX_K) == 8 * (4 * 16 * 272 + 2 * 256)
    for k, v in mine.items():
        assert v['lds'] == 8, (k, v)                                   # static: the block's weight counter
        assert v['lds'] + dsim.ds_lds_bytes(_lib.DEPTHCOV_MAX_K) <= 160 * 1024, (k, v)
        # the budget, as the listing has it: 12 accumulators of 8 registers, two operands, addresses.  next_free_vgpr
        # counts the unified file, accumulation registers included: 512 per SIMD lane, two waves of a workgroup's eight
        # per SIMD at 256
        assert v['vgpr'] <= 160, (k, v)
