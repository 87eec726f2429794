"""CPU tier of the cross-covariance of Vs(z) and the modelled data (bayhunter_amd/datacov.py, csrc/datacov_core.h,
csrc/datacov.hip):

* the restatement (tests/datacov_ref.py) is the cross block of np.cov on matrices that really are expanded;
* the host twin (tests/hostsim/datacov_sim.cpp: the core compiled with g++, the kernel's blocking, one fma chain per
  cell) agrees with the restatement within tests/datacov_tolerances.py, gives a set the same bits alone, at another offset
  and among other sets, and a column subset the same bits when the rows that count are the same;
* the host formulas of datacov.from_moments: a constant row, a constant column, a weight total of one row, a moved centre;
* bh_datacov_sets and the Python layer refuse bad arguments before they touch a device.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import datacov_ref as ref  # noqa: E402
import datacov_tolerances as tol  # noqa: E402

HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
SIM_SRCS = [os.path.join(HOSTSIM, 'datacov_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                          ('datacov_core.h', 'depthcov_core.h', 'posterior_core.h',
                                                           'stats_core.h', 'bh_common.h')]
SIM_SRCS.append(os.path.join(ROOT, 'include', 'bayhunter_amd.h'))
FMA = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
NAMES = ('C', 'r1x', 'r1y', 'qx', 'qy', 'total', 'excluded')
_vp = C.c_void_p


def load_sim():
    so = os.path.join(HOSTSIM, 'libdatacov_sim.so')
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SIM_SRCS):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + FMA + ['-o', so, SIM_SRCS[0]],
                       check=True)
    lib = C.CDLL(so)
    lib.dcs_datacov_sets.restype = C.c_int
    lib.dcs_datacov_sets.argtypes = [_vp, C.c_int, C.c_longlong, C.c_longlong, C.c_int, _vp, _vp, C.c_longlong, C.c_int, _vp,
                                     C.c_longlong, C.c_int, C.c_int, _vp, C.c_longlong, C.c_int, _vp, C.c_int, _vp,
                                     C.c_int] + [_vp] * 9 + [C.c_int]
    return lib


@pytest.fixture(scope='module')
def dsim():
    return load_sim()


def outputs(Z, K, S):
    """Arrays for bh_datacov_sets' outputs, filled with what no result is."""
    out = dict(C=np.full((Z, K, S), -7.), r1x=np.full((Z, K), -7.), r1y=np.full((Z, S), -7.), qx=np.full((Z, K), -7.),
               qy=np.full((Z, S), -7.), total=np.full(Z, -1, dtype=np.int64), excluded=np.full(Z, -1, dtype=np.int64))
    return out, [out[k].ctypes.data for k in NAMES]


def sim(dsim, c, block_rows=0, expect=0, cols=None):
    """The twin over a case's host arrays -> dict(C, r1x, r1y, qx, qy, total, excluded).  cols = (col0, S): those
    columns of the case's Y as the data columns."""
    rows = np.ascontiguousarray(c['rows'])
    assert rows.dtype in (np.float32, np.float64)
    w = None if c['weights'] is None else np.ascontiguousarray(c['weights'], dtype=np.int32)
    extra = None if c['extra'] is None else np.ascontiguousarray(c['extra'], dtype=np.float64)
    Y, err = np.ascontiguousarray(c['Y'], dtype=np.float64), np.ascontiguousarray(c['err'], dtype=np.int32)
    col0, S = (0, Y.shape[1]) if cols is None else cols
    start = np.ascontiguousarray(c['set_start'], dtype=np.int64)
    dep, cx, cy = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ('dep', 'cx', 'cy'))
    Z, nextra = start.size - 1, 0 if extra is None else extra.shape[1]
    assert cx.shape == (Z, dep.size + nextra) and cy.shape == (Z, S)
    out, ptrs = outputs(Z, dep.size + nextra, S)
    rc = dsim.dcs_datacov_sets(rows.ctypes.data, int(rows.dtype == np.float64), rows.shape[0], rows.shape[1], rows.shape[1],
                               None if w is None else w.ctypes.data, None if extra is None else extra.ctypes.data, nextra,
                               nextra, Y.ctypes.data, Y.shape[1], col0, S, err.ctypes.data if err.shape[1] else None,
                               err.shape[1], err.shape[1], start.ctypes.data, Z, dep.ctypes.data, dep.size, cx.ctypes.data,
                               cy.ctypes.data, *(ptrs + [block_rows]))
    assert rc == expect
    return out


def want_of(c):
    return ref.moments(c['rows'], c['weights'], c['extra'], c['Y'], c['err'], c['set_start'], c['dep'], c['cx'], c['cy'])


def same_bits(a, b, za=slice(None), zb=slice(None), what=''):
    for k in NAMES:
        assert np.asarray(a[k][za]).tobytes() == np.asarray(b[k][zb]).tobytes(), (what, k)


def sub_case(c, a, b, lead, z):
    """Rows a:b of a case, with the centres of its set z, behind `lead` other rows (the case's first ones, a set of
    their own with set 0's centres)."""
    sl = lambda x: None if x is None else np.ascontiguousarray(np.concatenate((x[:lead], x[a:b])))
    pick = [0, z] if lead else [z]
    return dict(rows=sl(c['rows']), weights=sl(c['weights']), extra=sl(c['extra']), Y=sl(c['Y']), err=sl(c['err']),
                dep=c['dep'], set_start=np.asarray(([0, lead] if lead else [0]) + [lead + b - a]), cx=c['cx'][pick],
                cy=c['cy'][pick])


# ---- the restatement ---------------------------------------------------------------------------------------------

def test_restatement_is_the_cross_block_of_numpy_cov_of_the_expanded_matrices():
    import depthcov_ref as dref
    rng = np.random.default_rng(5)
    rows = dref.random_rows(rng, 60, np.float32)
    rows[7] = np.nan
    w = rng.integers(0, 6, size=60)
    extra = rng.uniform(1.6, 1.9, size=(60, 2))
    dep = np.asarray([0., 3., 10., 25., 61.])
    Y = rng.normal(size=(60, 4)) + rows[:, :1].astype(np.float64)
    Y[11, 2] = np.nan
    err = np.zeros((60, 2), dtype=np.int32)
    err[13, 1] = 3
    w[[11, 13]] = 2
    X, has = dref.columns(rows, dep, extra)
    keep = (w > 0) & has
    keep[[11, 13]] = False
    ex, ey = np.repeat(X[keep], w[keep], axis=0), np.repeat(Y[keep], w[keep], axis=0)    # what the weights stand for
    want = np.cov(np.hstack((ex, ey)).T, bias=True)
    for cx, cy in ((ex.mean(axis=0), ey.mean(axis=0)), (ex.mean(axis=0) + 1e-3, ey.mean(axis=0) - 2e-3),
                   (np.zeros(7), np.zeros(4))):
        m = ref.moments(rows, w, extra, Y, err, [0, 60], dep, cx[None, :], cy[None, :])
        assert m['total'][0] == ex.shape[0] and m['terms'][0] == keep.sum()
        assert m['excluded'][0] == 4 + w[7] * (w[7] > 0)
        scale = np.sqrt(np.outer(np.diag(want)[:7], np.diag(want)[7:]))
        assert np.all(np.abs(ref.cov(m, 0).astype(np.float64) - want[:7, 7:]) <=
                      1e-12 * (scale + np.outer(np.abs(cx), np.abs(cy)) + 1))
        vx, vy = ref.variances(m, 0)
        assert np.allclose(vx.astype(np.float64), np.diag(want)[:7], rtol=0, atol=1e-12 * (1 + np.abs(cx).max() ** 2))
        assert np.allclose(vy.astype(np.float64), np.diag(want)[7:], rtol=0, atol=1e-12 * (1 + np.abs(cy).max() ** 2))


# ---- the twin ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fp64,weighted', [(False, True), (True, False)])
@pytest.mark.parametrize('ndep,nextra,S', [(2, 0, 1), (17, 1, 17), (33, 3, 40), (2, 0, 16), (17, 1, 257)])
def test_twin_agrees_with_the_restatement(dsim, ndep, nextra, S, fp64, weighted):
    from bayhunter_amd import _lib
    B = dsim.dcs_block_rows()
    assert B == _lib.DEPTHCOV_BLOCK_ROWS and dsim.dcs_max_k() == _lib.DEPTHCOV_MAX_K
    assert dsim.dcs_max_s() == _lib.DATACOV_MAX_S >= 1024
    c = ref.case(B, ndep, nextra, S, fp64, weighted)
    want = want_of(c)
    assert want['total'][2] == 0 and want['total'][5] == 0 and np.all(want['total'][[0, 1, 3, 4, 6, 7]] > 0)
    assert want['excluded'][5] == (0 if weighted else 5) and want['excluded'][7] > 0
    got = sim(dsim, c)
    worst = tol.check_moments(got, want, 'ndep %d nextra %d S %d' % (ndep, nextra, S))
    print('ndep %d nextra %d S %d fp64 %d weighted %d: worst |difference| / bound %.3g' % (ndep, nextra, S, fp64, weighted,
                                                                                           worst))


def test_twin_set_independence(dsim):
    """A set alone, at another offset in rows, gives the bits it has in the joint call; two runs agree."""
    c = ref.case(dsim.dcs_block_rows(), 17, 1, 17, False, True)
    got = sim(dsim, c)
    same_bits(got, sim(dsim, c))
    st = c['set_start']
    for z in range(len(st) - 1):
        a, b = int(st[z]), int(st[z + 1])
        if a == b:
            continue
        same_bits(sim(dsim, sub_case(c, a, b, 0, z)), got, slice(0, 1), slice(z, z + 1), z)
        same_bits(sim(dsim, sub_case(c, a, b, 3, z)), got, slice(1, 2), slice(z, z + 1), z)


def test_twin_blocks_add_up_in_order(dsim):
    """With blocks of 4 rows the result is the fold of the 4-row partials in ascending order, from 0.0."""
    c = ref.case(dsim.dcs_block_rows(), 2, 1, 3, True, True)
    a, b = int(c['set_start'][3]), int(c['set_start'][4]) + 7          # the set of 4 rows and 7 of the next: 11 rows
    one = sub_case(c, a, b, 0, 4)
    got = sim(dsim, one, block_rows=4)
    acc = {k: np.zeros_like(got[k]) for k in NAMES}
    for r0 in range(a, b, 4):
        part = sim(dsim, sub_case(c, r0, min(r0 + 4, b), 0, 4), block_rows=4)
        acc = {k: acc[k] + part[k] for k in NAMES}
    same_bits(got, acc)
    assert got['total'][0] > 0


def test_twin_column_subset_keeps_its_bits(dsim):
    """Without NaN rows the rows that count do not depend on the columns: the cells of a column subset are the bits of
    the whole when Y holds that subset alone -- and with NaN rows in another column they are not the same rows."""
    c = ref.case(dsim.dcs_block_rows(), 17, 1, 40, False, True, nans=False)
    got = sim(dsim, c)
    sub = sim(dsim, dict(c, cy=c['cy'][:, 5:19]), cols=(5, 14))
    narrow = sim(dsim, dict(c, Y=np.ascontiguousarray(c['Y'][:, 5:19]), cy=c['cy'][:, 5:19]))
    for part in (sub, narrow):
        assert part['C'].tobytes() == np.ascontiguousarray(got['C'][:, :, 5:19]).tobytes()
        for k in ('r1y', 'qy'):
            assert part[k].tobytes() == np.ascontiguousarray(got[k][:, 5:19]).tobytes(), k
        for k in ('r1x', 'qx', 'total', 'excluded'):
            assert part[k].tobytes() == got[k].tobytes(), k
    holes = ref.case(dsim.dcs_block_rows(), 17, 1, 40, False, True, nans=True)
    whole, part = sim(dsim, holes), sim(dsim, dict(holes, cy=holes['cy'][:, :39]), cols=(0, 39))
    assert np.all(part['total'][[6, 7]] > whole['total'][[6, 7]]) and np.all(part['excluded'] <= whole['excluded'])


def test_geometry(dsim):
    """The groups of data-column tiles: as many tiles as the workgroup's 96 accumulators take beside Tx model tiles, 16
    at most; 201 depths and an extra with 222 data columns are two groups of 7 tiles, all 182 tile pairs in use."""
    assert [dsim.dcs_group_cols(K) for K in (1, 16, 17, 36, 96, 97, 202, 256)] == [256, 256, 256, 256, 256, 208, 112, 96]
    assert -(-222 // dsim.dcs_group_cols(202)) == 2
    # two stages of ex and dy and one of dx, 16 rows each at a pitch off the 32-bank stride, the grid and the centres
    assert dsim.dcs_lds_bytes(202) == 8 * (16 * (3 * 208 + 2 * 112) + 2 * 208 + 112)
    assert dsim.dcs_lds_bytes(256) == 8 * (16 * (3 * 272 + 2 * 112) + 2 * 256 + 96)
    assert dsim.dcs_max_lds_bytes() == max(dsim.dcs_lds_bytes(K) for K in range(1, 257)) <= 160 * 1024 - 256


# ---- the host formulas ------------------------------------------------------------------------------------------------

def test_from_moments_is_the_restatements_covariance(dsim):
    from bayhunter_amd import datacov as dc
    c = ref.case(dsim.dcs_block_rows(), 17, 1, 17, True, True)
    want, got = want_of(c), sim(dsim, c)
    moved = dict(c, cx=c['cx'] + 1e-3, cy=c['cy'] - 2e-3)
    want_m, got_m = want_of(moved), sim(dsim, moved)
    tol.check_moments(got_m, want_m, 'moved centres')
    for z in np.nonzero(got['total'] > 0)[0]:
        arg = lambda g: [g[k][z] for k in ('C', 'r1x', 'r1y', 'qx', 'qy', 'total')]
        cov, corr, std_x, std_y = dc.from_moments(*arg(got))
        assert np.all(np.abs(cov - ref.cov(want, z)) <= tol.cov_bound(want, z)), z
        vx, vy = ref.variances(want, z)
        bx, by = tol.var_bounds(want, z)
        for std, v, b in ((std_x, vx, bx), (std_y, vy, by)):
            live = std > 0
            assert np.all(np.abs(std[live] ** 2 - v[live]) <= b[live] + 4 * tol.U * np.abs(v[live])), z
            assert np.all(np.abs(v[~live]) <= b[~live]), z                # a variance held at 0 was 0 to its bound
        # the centres moved: the same covariance, to the bound of both (not bit for bit)
        covm = dc.from_moments(*arg(got_m))[0]
        both = tol.cov_bound(want, z, recentred=True) + tol.cov_bound(want_m, z, recentred=True)
        flat = np.isnan(corr)
        assert np.all((np.abs(covm.astype(np.longdouble) - cov) <= both) | flat), (z, np.abs(covm - cov).max(), both.max())
    with pytest.raises(ValueError):
        dc.from_moments(np.zeros((2, 3)), np.zeros(2), np.zeros(3), np.zeros(2), np.zeros(3), 0)
    with pytest.raises(ValueError):
        dc.from_moments(np.zeros((2, 2)), np.zeros(2), np.zeros(3), np.zeros(2), np.zeros(3), 5)
    with pytest.raises(ValueError):
        dc.from_moments(np.zeros((2, 3)), np.zeros(2), np.zeros(3), np.zeros(3), np.zeros(3), 5)


def test_from_moments_rules():
    from bayhunter_amd import datacov as dc
    rng = np.random.default_rng(3)
    X, Y = rng.normal(size=(50, 4)), rng.normal(size=(50, 3))
    Y[:, 0] += X[:, 1]
    X[:, 2] = 3.5                                                     # a model column of one value
    Y[:, 1] = -2.25                                                   # a datum every model agrees on
    w = rng.integers(1, 5, size=50).astype(np.float64)

    def moments(cx, cy, rows=slice(None)):
        dx, dy, ww = X[rows] - cx, Y[rows] - cy, w[rows, None]
        return ((ww * dx).T @ dy, (ww * dx).sum(axis=0), (ww * dy).sum(axis=0), (ww * dx * dx).sum(axis=0),
                (ww * dy * dy).sum(axis=0), w[rows].sum())
    cx, cy = np.asarray([0.1, -0.2, 3.5, 0.]), np.asarray([0.3, -2.25, 0.])
    cov, corr, std_x, std_y = dc.from_moments(*moments(cx, cy))
    assert cov.shape == corr.shape == (4, 3) and std_x.shape == (4,) and std_y.shape == (3,)
    assert std_x[2] == 0 and not np.any(cov[2]) and np.all(np.isnan(corr[2]))
    assert std_y[1] == 0 and not np.any(cov[:, 1]) and np.all(np.isnan(corr[:, 1]))
    lx, ly = [0, 1, 3], [0, 2]
    assert np.all(np.isfinite(corr[np.ix_(lx, ly)])) and np.all(np.abs(corr[np.ix_(lx, ly)]) <= 1)
    ex, ey = np.repeat(X, w.astype(int), axis=0), np.repeat(Y, w.astype(int), axis=0)
    full = np.cov(np.hstack((ex, ey)).T, bias=True)
    assert np.allclose(cov, full[:4, 4:], rtol=0, atol=1e-13)
    assert np.allclose(std_x, np.sqrt(np.diag(full)[:4]), rtol=0, atol=1e-13)
    assert np.allclose(std_y, np.sqrt(np.diag(full)[4:]), rtol=0, atol=1e-13)
    fc = np.corrcoef(np.hstack((ex[:, lx], ey[:, ly])).T)
    assert np.allclose(corr[np.ix_(lx, ly)], fc[:3, 3:], rtol=0, atol=1e-12) and corr[1, 0] > 0.5
    # centres off the constant columns' values by a rounding: constant_x / constant_y hold the variances at 0
    cov2, corr2, sx2, sy2 = dc.from_moments(*moments(cx + [0, 0, 4.4e-16, 0], cy - [0, 4.4e-16, 0]),
                                            constant_x=[False, False, True, False], constant_y=[False, True, False])
    assert sx2[2] == 0 and sy2[1] == 0 and not np.any(cov2[2]) and not np.any(cov2[:, 1])
    assert np.all(np.isnan(corr2[2])) and np.all(np.isnan(corr2[:, 1]))
    # moved centres: the same covariance to rounding
    cov3 = dc.from_moments(*moments(cx + 1e-3, cy - 2e-3))[0]
    assert np.allclose(cov3, cov, rtol=0, atol=1e-14)
    # one row: W is its weight, no variance anywhere, every correlation NaN
    cov1, corr1, sx1, sy1 = dc.from_moments(*moments(X[4], Y[4], slice(4, 5)))
    assert not np.any(cov1) and not np.any(sx1) and not np.any(sy1) and np.all(np.isnan(corr1))


# ---- the library ------------------------------------------------------------------------------------------

def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    nodev = C.c_void_p(16)                  # never dereferenced: the arguments are checked first
    dep0 = np.asarray([0., 1., 2.])
    out, ptrs = outputs(2, 4, 5)
    host = dict(cx=np.zeros((2, 4)), cy=np.zeros((2, 5)))

    def call(rows=nodev, nrows=10, stride=12, width=12, extra=nodev, extra_stride=1, nextra=1, Y=nodev, y_stride=9, col0=2,
             S=5, err=nodev, err_stride=2, nflags=2, start=(0, 4, 10), nsets=2, dep=dep0, ndep=3, null=None):
        st = None if start is None else np.asarray(start, dtype=np.int64)
        p = lambda a: None if a is None else a.ctypes.data
        tail = [p(host['cx']), p(host['cy'])] + list(ptrs)
        if null is not None:
            tail[null] = None
        return lib.bh_datacov_sets(rows, 0, nrows, stride, width, None, extra, extra_stride, nextra, Y, y_stride, col0, S,
                                   err, err_stride, nflags, p(st), nsets, p(dep), ndep, *(tail + [None]))
    msg = lambda: lib.bh_last_error()
    assert call(rows=None) == E and call(nrows=0, start=(0, 0, 0)) == E and b'empty' in msg()
    assert call(nrows=(1 << 32) + 1, start=(0, 4, (1 << 32) + 1)) == E and b'2^32' in msg()
    assert call(stride=11) == E and b'stride' in msg() and call(width=1) == E
    assert call(ndep=0) == E and b'ndep' in msg() and call(dep=None) == E
    assert call(dep=np.asarray([0., 2., 1.])) == E and b'ascending' in msg()
    assert call(nextra=-1) == E and call(extra=None) == E and b'extra' in msg() and call(extra_stride=0) == E
    big = np.arange(_lib.DEPTHCOV_MAX_K, dtype=np.float64)
    assert call(dep=big, ndep=big.size) == E and b'above 256' in msg()
    assert call(S=0) == E and b'data columns' in msg() and call(S=_lib.DATACOV_MAX_S + 1, y_stride=4096) == E
    assert call(Y=None) == E and b'y_stride' in msg() and call(col0=-1) == E and call(y_stride=6) == E
    assert call(nflags=-1) == E and b'err' in msg() and call(err=None) == E and call(err_stride=1) == E
    assert call(nsets=0) == E and b'one set' in msg()
    assert call(start=None) == E
    assert call(start=(0, 6, 4, 10), nsets=3) == E and b'ascending' in msg()
    assert call(start=(0, 4, 9)) == E and b'end at nrows' in msg() and call(start=(1, 4, 10)) == E
    for i in range(9):
        assert call(null=i) == E and b'cx, cy, C' in msg(), i
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read()
    assert '#define BH_DATACOV_MAX_S %d' % _lib.DATACOV_MAX_S in header and 'int  bh_datacov_sets(' in header
    assert 'datacov.hip' in _lib.SOURCES and 'datacov_core.h' in _lib.HEADERS and 'bh_datacov_sets' in _lib.EXPORTS


def test_python_layer_refuses_bad_arguments():
    from bayhunter_amd import datacov as dc
    models = np.zeros((10, 12), dtype=np.float32)
    tg = object()                                                      # never looked at: the arguments are checked first
    with pytest.raises(ValueError, match='set_start'):
        dc.summarize_sets([tg, tg, tg], models, [0, 6, 4, 10], 1.73, device='cpu')
    with pytest.raises(ValueError, match='one JointTarget per set'):
        dc.summarize_sets([tg], models, [0, 4, 10], 1.73, device='cpu')
    with pytest.raises(ValueError, match='dep_int'):
        dc.summarize(tg, models, 1.73, dep_int=[0., 2., 1.], device='cpu')
    with pytest.raises(ValueError, match='dep_int'):
        dc.summarize(tg, models, 1.73, dep_int=[], device='cpu')
    with pytest.raises(ValueError, match='extra'):
        dc.summarize(tg, models, 1.73, extra=np.zeros((9, 1)), extra_names=('a',), device='cpu')
    with pytest.raises(ValueError, match='extra_names'):
        dc.summarize(tg, models, 1.73, extra=np.zeros((10, 2)), extra_names=('a',), device='cpu')
    with pytest.raises(ValueError, match='at most'):
        dc.summarize(tg, models, 1.73, dep_int=np.arange(256.), extra=np.zeros((10, 1)), extra_names=('a',), device='cpu')
    with pytest.raises(ValueError, match='one weight per row'):
        dc.summarize(tg, models, 1.73, weights=np.ones(9, dtype=np.int32), device='cpu')
    with pytest.raises(ValueError, match='vpvs'):
        dc.summarize(tg, models, np.full(9, 1.73), device='cpu')
    with pytest.raises(ValueError, match='rf_p'):
        dc.summarize_sets([tg, tg], models, [0, 4, 10], 1.73, rf_p=np.zeros((3, 1)), device='cpu')
    with pytest.raises(ValueError, match='max_rows'):
        dc.summarize_sets([tg, tg], models, [0, 4, 10], 1.73, max_rows=0, device='cpu')
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool, StationView
    assert callable(ChainPool.data_covariance) and callable(StationPool.data_covariance)
    assert StationView.data_covariance is ChainPool.data_covariance and 'data_covariance()' in StationView.__doc__
