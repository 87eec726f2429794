"""CPU tier of the depth-binned receiver-function sensitivity statistics (csrc/rf_sens_sets_core.h, csrc/rf_sens_sets.hip,
bh_rf_sens_sets_*):

* the host twin (tests/hostsim/rf_sens_sets_sim.cpp: the kernel's core compiled with g++, the tile, the register blocking
  and the sums in the kernel's order) lies within the derived bounds (tests/rf_sens_sets_tolerances.py) of the longdouble
  restatement (tests/rf_sens_sets_ref.py), on synthetic K with mixed signs, garbage behind nlay and in the strides, rows
  without a trace, for all four kinds and three selections;
* at 1 and 5 selected samples it equals tests/hostsim/sens_sets_sim.cpp bit for bit;
* many sets in one call equal the per-set calls bit for bit;
* the C ABI refuses bad arguments before a device is touched.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import rf_sens_sets_ref as ref  # noqa: E402
import rf_sens_sets_tolerances as tol  # noqa: E402
import test_sens_sets as base  # noqa: E402

HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
KINDS = base.KINDS
LMAX, NOUT = 8, 80
FIELDS = ('total', 'excluded', 's1', 's2', 'vmin', 'vmax')
# all 80 samples (five tiles of 16), a window of 5 (a thread's second group holds one sample), every third (27: a tile
# of 11), one sample, and 67 scattered ones (four tiles and three samples)
SELECTIONS = {'all': None, 'window': np.arange(33, 38), 'third': np.arange(0, NOUT, 3), 'one': np.array([79]),
              '67': np.sort(np.random.RandomState(5).choice(NOUT, 67, replace=False))}


def load_sim():
    so = os.path.join(HOSTSIM, 'librf_sens_sets_sim.so')
    srcs = [os.path.join(HOSTSIM, 'rf_sens_sets_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                              ('rf_sens_sets_core.h', 'sens_sets_core.h', 'bh_common.h')]
    srcs.append(os.path.join(ROOT, 'include', 'bayhunter_amd.h'))
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + base.FMA + ['-o', so, srcs[0]],
                       check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.rss_sets.restype = C.c_int
    lib.rss_sets.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, vp,
                             vp, C.c_int, vp, C.c_longlong, vp, C.c_int, vp] + [vp] * 6
    lib.rss_lds_bytes.argtypes = [C.c_int]
    return lib


@pytest.fixture(scope='module')
def rsim():
    return load_sim()


@pytest.fixture(scope='module')
def ssim():
    return base.load_sim()


def make_case(seed, R, Lmax=LMAX, nout=NOUT, nan_rows=True, kpad=5, rfpad=3, built=True):
    """test_sens_sets.make_case with a trace's samples for periods -> dict(nlay, h, q, w as there; K [R, nout*4*Lmax + kpad]
    with garbage in the stride; rf [R, nout + rfpad] likewise) plus '_K' [R, nout, 4, Lmax], the view of K.  The rows that
    case makes NaN at one period are, with nan_rows, rows without a trace (K and rf NaN throughout), else whole."""
    c = base.make_case(seed, R, Lmax=Lmax, nper=nout, built=built)
    rs = np.random.RandomState(seed + 1000)
    K = c['K']
    for r in range(R):
        if r % 7 == 3:
            n = min(max(int(c['nlay'][r]), 0), Lmax)
            K[r] = rs.standard_normal((nout, 4, Lmax)) * 0.1
            K[r, :, :, n:] = np.nan if r % 2 else 1e30
            if nan_rows:
                K[r] = np.nan
    rf = np.full((R, nout + rfpad), 1e30)
    rf[:, :nout] = rs.standard_normal((R, nout))
    rf[::2, nout:] = np.nan
    if nan_rows:
        rf[3::7, :nout] = np.nan
    Kp = np.full((R, nout * 4 * Lmax + kpad), np.nan)
    Kp[1::2, nout * 4 * Lmax:] = 1e30
    Kp[:, :nout * 4 * Lmax] = K.reshape(R, -1)
    return dict(nlay=c['nlay'], h=c['h'], q=c['q'], w=c['w'], K=np.ascontiguousarray(Kp), rf=np.ascontiguousarray(rf))


def view_K(case, Lmax=LMAX):
    nout = (case['K'].shape[1]) // (4 * Lmax)
    return case['K'][:, :nout * 4 * Lmax].reshape(case['K'].shape[0], nout, 4, Lmax)


def rows_of(case, a, b):
    return {k: v[a:b] for k, v in case.items()}


def blank(Z, nsel, cells):
    out = dict(total=np.zeros(Z, dtype=np.int64), excluded=np.zeros(Z, dtype=np.int64))
    for k in FIELDS[2:]:
        out[k] = np.zeros((Z, nsel, cells))
    return out


def twin(rsim, case, start, samples, edges, kind, weights=True, drho=0.32, Lmax=LMAX, nout=NOUT):
    """The host twin -> bh_rf_sens_sets_finish's arrays."""
    start = np.ascontiguousarray(start, dtype=np.int64)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    smp = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32)
    Z, nsel = start.size - 1, nout if smp is None else smp.size
    assert start[-1] == case['K'].shape[0]
    out = blank(Z, nsel, edges.size)
    arr = {k: np.ascontiguousarray(v) for k, v in case.items()}
    q = arr['q'] if kind == 'vs_total' else None
    rc = rsim.rss_sets(start.ctypes.data, Z, nout, None if smp is None else smp.ctypes.data, nsel, edges.ctypes.data,
                       edges.size, ref.KINDS[kind], drho, Lmax, arr['h'].shape[1], arr['nlay'].ctypes.data,
                       arr['h'].ctypes.data, None if q is None else q.ctypes.data, 0 if q is None else q.shape[1],
                       arr['K'].ctypes.data, arr['K'].shape[1], arr['rf'].ctypes.data, arr['rf'].shape[1],
                       arr['w'].ctypes.data if weights else None, *[out[k].ctypes.data for k in FIELDS])
    assert rc == 0
    return out


def errors_over_bounds(got, z, want, Lmax):
    """Set z of the sums `got` against the restatement `want` -> (worst |mean error| / bound, worst |variance error| /
    bound); counts and NaN patterns must agree."""
    assert got['total'][z] == want['total'] and got['excluded'][z] == want['excluded']
    if not want['total']:
        assert np.isnan(got['vmin'][z]).all() and np.isnan(got['vmax'][z]).all()
        assert not got['s1'][z].any() and not got['s2'][z].any()
        return 0., 0.
    assert not np.isnan(got['vmin'][z]).any()
    W = float(got['total'][z])
    mean = got['s1'][z] / W
    var = got['s2'][z] / W - mean * mean
    worst = []
    for val, name, bound in ((mean, 'mean', tol.mean_bound(want['n'], Lmax, want['absmean'])),
                             (var, 'var', tol.var_bound(want['n'], Lmax, want['sqmean']))):
        err = np.abs(val.astype(np.longdouble) - want[name]).astype(np.float64)
        worst.append(float(np.where(err == 0, 0., err / np.where(err == 0, 1., bound)).max()))
    return tuple(worst)


def assert_same_bits(a, b):
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('sel', ['all', 'window', 'third'])
def test_twin_lies_within_the_bounds_of_the_restatement(rsim, sel, kind):
    case, samples = make_case(61, 300), SELECTIONS[sel]
    assert case['nlay'].min() == 1 and case['nlay'].max() == LMAX + 1 and (case['w'] == 0).sum() > 10
    assert np.isnan(case['rf'][:, 0]).sum() > 10
    sizes = [4, 1, 0, 295]                             # the built geometries alone, one row, none, all the rest
    start = np.concatenate(([0], np.cumsum(sizes)))
    K = view_K(case)
    worst = [0., 0.]
    for grid in sorted(base.EDGES):
        edges = base.EDGES[grid]
        got = twin(rsim, case, start, samples, edges, kind)
        for z in range(len(sizes)):
            r = rows_of(case, start[z], start[z + 1])
            want = ref.summarize(r['nlay'], r['h'], r['q'], K[start[z]:start[z + 1]], r['rf'], r['w'], samples, edges, kind)
            e = errors_over_bounds(got, z, want, LMAX)
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        assert got['total'][2] == 0 and got['excluded'][2] == 0 and got['excluded'][3] > 0
    print('%s %s: worst error / bound: mean %.3g, variance %.3g' % (sel, kind, worst[0], worst[1]))
    assert worst[0] <= 1. and worst[1] <= 1., worst


@pytest.mark.parametrize('sel', ['one', 'window'])
def test_twin_equals_the_sens_sets_twin_bit_for_bit(rsim, ssim, sel):
    """1 and 5 selected samples of rows that all have a trace: bh_sens_sets_*'s sums for the same K with a finite c_out."""
    case, samples = make_case(62, 1300, nan_rows=False), SELECTIONS[sel]
    assert samples.size in (1, 5)
    sizes = [0, 1, 255, 256, 257, 513, 18]
    start = np.concatenate(([0], np.cumsum(sizes)))
    case['w'][start[1]] = 2
    case['w'][start[6]:] = 0
    other = dict(nlay=case['nlay'], h=case['h'], q=case['q'], w=case['w'],
                 K=np.ascontiguousarray(view_K(case)[:, samples]), c=np.full((1300, samples.size), 3.))
    for kind in KINDS:
        for edges in (base.EDGES['fine'], base.EDGES['one']):
            got = twin(rsim, case, start, samples, edges, kind)
            want = base.twin(ssim, other, start, edges, kind)
            for k in FIELDS[2:]:
                assert_same_bits(got[k], want[k])
            for k in FIELDS[:2]:
                assert np.array_equal(got[k][:, None] * np.ones(samples.size, dtype=np.int64), want[k])
    assert got['total'][5] > 0 and got['excluded'][5] > 0


def test_sets_equal_their_rows_alone_and_min_max_are_exact(rsim):
    case, edges, samples = make_case(63, 1300), base.EDGES['fine'], SELECTIONS['67']
    sizes = [0, 1, 255, 256, 257, 513, 18]
    start = np.concatenate(([0], np.cumsum(sizes)))
    case['w'][start[1]] = 2
    case['w'][start[6]:] = 0
    got = twin(rsim, case, start, samples, edges, 'vs_total')
    for z, n in enumerate(sizes):
        a, b = start[z], start[z + 1]
        alone = twin(rsim, rows_of(case, a, b) if n else rows_of(case, 0, 1), [0, n] if n else [0, 0, 1], samples, edges,
                     'vs_total')
        for k in FIELDS:
            assert_same_bits(got[k][z], alone[k][0])
    for z in (0, 6):
        assert not got['total'][z] and np.isnan(got['vmin'][z]).all() and not got['s1'][z].any()
    assert not got['excluded'][6]                    # weight 0 is not excluded weight
    # every row of the largest set as a set of its own without weights: s1 is then the row's cell, to the bit
    z = 5
    a, b = start[z], start[z + 1]
    one = twin(rsim, rows_of(case, a, b), np.arange(b - a + 1), samples, edges, 'vs_total', weights=False)
    counts = (one['total'] > 0) & (case['w'][a:b] > 0)
    x = one['s1'][counts]
    assert np.array_equal(x.min(axis=0), got['vmin'][z]) and np.array_equal(x.max(axis=0), got['vmax'][z])
    assert np.array_equal(one['vmin'][counts], x) and np.array_equal(one['vmax'][counts], x)
    # the selection picks cells: the full result at the selected samples
    full = twin(rsim, case, start, None, edges, 'vs_total')
    for k in FIELDS[2:]:
        assert_same_bits(np.ascontiguousarray(full[k][:, samples]), got[k])


def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    edges = base.EDGES['fine'].copy()
    err = lambda: lib.bh_last_error()

    def create(start=(0, 4, 10), nsets=2, nout=NOUT, samples=None, nsel=0, e=edges, ne=None, kind=4, drho=0.32, keep=False):
        h = C.c_void_p(77)
        start = None if start is None else np.asarray(start, dtype=np.int64)
        smp = None if samples is None else np.asarray(samples, dtype=np.int32)
        rc = lib.bh_rf_sens_sets_create(C.byref(h), None if start is None else start.ctypes.data, nsets, nout,
                                        None if smp is None else smp.ctypes.data, nsel if smp is None else smp.size,
                                        None if e is None else e.ctypes.data, (0 if e is None else e.size) if ne is None else ne,
                                        kind, drho, None)
        if rc != _lib.BH_OK:
            assert not h.value                       # no handle comes back with an error
        elif keep:
            return h
        else:
            lib.bh_rf_sens_sets_destroy(h)
        return rc
    # bh_sens_sets_create's refusals
    assert create(nsets=0) == E and b'sets' in err() and create(nsets=_lib.PAIRS_MAX_SETS + 1) == E
    assert create(start=None) == E and create(start=(1, 4, 10)) == E and b'begin at 0' in err()
    assert create(start=(0, 6, 4, 10), nsets=3) == E and b'ascending' in err()
    assert create(e=None) == E and create(ne=1) == E and b'depth edges' in err()
    assert create(e=np.arange(_lib.SENS_SETS_MAX_BINS + 2.)) == E and b'depth edges' in err()
    assert create(e=edges[::-1].copy()) == E and b'ascending' in err()
    bad = edges.copy()
    bad[-1] = np.inf
    assert create(e=bad) == E and b'finite' in err()
    for kind in (0, 5, -1):
        assert create(kind=kind) == E and b'kind' in err()
    assert create(drho=np.nan) == E and b'drho_dvp' in err()
    # its own: nout, the samples, the budget
    assert create(nout=0) == E and b'nout' in err() and create(nout=_lib.RF_SENS_SETS_MAX_SAMPLES + 1) == E and b'nout' in err()
    assert create(samples=[]) == E and b'nsel' in err() and create(samples=np.arange(NOUT + 1)) == E
    assert create(samples=[0, NOUT]) == E and b'out of range' in err() and create(samples=[-1, 3]) == E and b'out of range' in err()
    assert create(samples=[3, 3]) == E and b'ascending' in err() and create(samples=[5, 4]) == E and b'ascending' in err()
    assert create(samples=[0, 5, NOUT - 1]) == _lib.BH_OK and create() == _lib.BH_OK        # (create touches no device)
    many = np.arange(0, 60001, 10000, dtype=np.int64)                                       # 6 sets
    big = np.linspace(0., 100., 1025)
    cells = 6 * 4096 * 1025 * 32
    assert cells < _lib.RF_SENS_SETS_MAX_ACC_BYTES and create(start=many, nsets=6, nout=4096, e=big) == _lib.BH_OK
    many = np.arange(0, 90001, 10000, dtype=np.int64)                                       # 9 sets: 1.18e9 bytes
    assert 9 * 4096 * 1025 * 32 > _lib.RF_SENS_SETS_MAX_ACC_BYTES
    assert create(start=many, nsets=9, nout=4096, e=big) == E and b'BH_RF_SENS_SETS_MAX_ACC_BYTES' in err()
    assert create(start=many, nsets=9, nout=4096, samples=np.arange(0, 4096, 2), e=big) == _lib.BH_OK      # the selection counts
    # add: checked before the device is touched, so without one
    h = create(start=(0, 256, 300), keep=True)
    nodev = C.c_void_p(16)
    row = NOUT * 4 * LMAX

    def add(handle=h, row0=0, B=256, Lmax=LMAX, ms=11, nlay=nodev, hthk=nodev, q=nodev, qs=10, K=nodev, ks=row + 5, rf=nodev,
            rs=NOUT + 3):
        return lib.bh_rf_sens_sets_add(handle, row0, B, Lmax, ms, nlay, hthk, q, qs, K, ks, rf, rs, None)
    try:
        assert add(handle=None) == E and b'handle' in err()
        assert add(ks=row - 1) == E and b'k_stride' in err() and add(rs=NOUT - 1) == E and b'rf_stride' in err()
        assert add(row0=1) == E and b'ascending order' in err() and add(B=301) == E and b'more rows' in err()
        assert add(q=None) == E and b'needs q' in err() and add(qs=7) == E and add(ms=7) == E and b'model_stride' in err()
        assert add(Lmax=0) == E and add(Lmax=101) == E and add(B=-1) == E and b'B/Lmax' in err()
        assert add(K=None) == E and add(rf=None) == E and add(nlay=None) == E and b'NULL pointer' in err()
        assert add(B=100) == E and b'multiple of BH_SENS_SETS_BLOCK_ROWS' in err()
        assert add(B=0) == _lib.BH_OK
        assert lib.bh_rf_sens_sets_finish(h, None, None, None, None, None, None) == E and b'not all rows' in err()
    finally:
        lib.bh_rf_sens_sets_destroy(h)
    assert lib.bh_rf_sens_sets_finish(None, None, None, None, None, None, None) == E and b'handle' in err()
    lib.bh_rf_sens_sets_destroy(None)
    # a handle whose sets are all empty finishes without a device: no weight, sums 0, min and max NaN
    h = create(start=(0, 0, 0), samples=[1, 2], e=np.array([0., 1., 2.]), keep=True)
    out = blank(2, 2, 3)
    out['s1'][:] = 7.
    try:
        assert lib.bh_rf_sens_sets_finish(h, *[out[k].ctypes.data for k in FIELDS]) == _lib.BH_OK
    finally:
        lib.bh_rf_sens_sets_destroy(h)
    assert not out['total'].any() and not out['s1'].any() and np.isnan(out['vmin']).all() and np.isnan(out['vmax']).all()
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read()
    assert '#define BH_RF_SENS_SETS_MAX_SAMPLES   %d' % _lib.RF_SENS_SETS_MAX_SAMPLES in header
    assert '#define BH_RF_SENS_SETS_MAX_ACC_BYTES (1ll << 30)' in header and _lib.RF_SENS_SETS_MAX_ACC_BYTES == 1 << 30
    assert 'rf_sens_sets.hip' in _lib.SOURCES and 'rf_sens_sets_core.h' in _lib.HEADERS and 'sens_sets_host.h' in _lib.HEADERS
    for f in ('create', 'add', 'finish', 'destroy'):
        assert 'bh_rf_sens_sets_' + f in _lib.EXPORTS
