"""CPU tier of the depth-binned sensitivity statistics (bayhunter_amd/sensitivity.py, csrc/sens_sets_core.h,
csrc/sens_sets.hip):

* the host twin (tests/hostsim/sens_sets_sim.cpp: the kernel's core compiled with g++, the sums in the kernel's order)
  lies within the derived bounds (tests/sens_sets_tolerances.py) of the longdouble restatement on the expanded matrix
  (tests/sens_sets_ref.py), on synthetic K with mixed signs and garbage behind nlay, over the bin geometries where the
  walk can go wrong, for all four kinds;
* min and max are exactly the least and the largest of the rows' own cells;
* many sets in one call equal the per-set calls bit for bit;
* the bins and the half-space add up to the layers when the edges cover the stack;
* from_sums' rules, split_runs' cuts, and the refusals of the library and of the Python layer before a device is touched.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sens_sets_ref as ref  # noqa: E402
import sens_sets_tolerances as tol  # noqa: E402

HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
FMA = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
KINDS = ('vp', 'vs', 'rho', 'vs_total')
LMAX = 8
# nb = 1 with the first edge above 0; 67 bins of 0.5 km from 0; edges that fall on the built rows' interfaces
EDGES = {'one': np.array([1.5, 40.]), 'fine': 0.5 * np.arange(68), 'coarse': np.array([2., 3., 5., 10., 20., 23.75, 60.])}
FIELDS = ('total', 'excluded', 's1', 's2', 'vmin', 'vmax')


def load_sim():
    so = os.path.join(HOSTSIM, 'libsens_sets_sim.so')
    srcs = [os.path.join(HOSTSIM, 'sens_sets_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                           ('sens_sets_core.h', 'bh_common.h')]
    srcs.append(os.path.join(ROOT, 'include', 'bayhunter_amd.h'))
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + FMA + ['-o', so, srcs[0]],
                       check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.sss_sets.restype = C.c_int
    lib.sss_sets.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, vp, vp, C.c_int,
                             vp, vp, vp] + [vp] * 6
    lib.sss_lds_bytes.argtypes = [C.c_int] * 3
    return lib


@pytest.fixture(scope='module')
def ssim():
    return load_sim()


def make_case(seed, R, Lmax=LMAX, nper=5, pad=3, built=True):
    """Synthetic rows: dict(nlay [R], h [R, Lmax + pad], q [R, Lmax + pad - 1], K [R, nper, 4, Lmax], c [R, nper], w [R])
    with K random and of mixed signs, garbage (NaN, 1e30) behind nlay and in the strides, weights 0 .. 5, some rows NaN in
    one period only, some with nlay 1 and Lmax + 1 -- and, with `built`, the geometries of built_rows() in rows 0 .. 3."""
    rs = np.random.RandomState(seed)
    nlay = rs.randint(2, Lmax + 1, R).astype(np.int32)
    h = rs.uniform(0.2, 9., (R, Lmax + pad))
    q = rs.uniform(1.6, 1.95, (R, Lmax + pad - 1))
    K = rs.standard_normal((R, nper, 4, Lmax)) * 10. ** rs.uniform(-3, 0, (R, nper, 1, 1))
    c = rs.uniform(2., 4.5, (R, nper))
    w = rs.randint(0, 6, R).astype(np.int32)
    if built and R >= 4:
        for r, hs in enumerate(built_rows(Lmax)):
            nlay[r] = len(hs) + 1
            h[r, :len(hs)] = hs
            w[r] = r + 1
    for r in range(R):
        if r % 11 == 5:
            h[r, rs.randint(0, nlay[r] - 1) if nlay[r] > 2 else 0] = 0.          # a layer without thickness
        if r % 13 == 7:
            nlay[r] = 1 if r % 2 else Lmax + 1                                   # no model
        if r % 7 == 3:
            p = rs.randint(0, nper)
            c[r, p] = np.nan
            K[r, p] = np.nan                                                     # no value at one period only
    for r in range(R):
        n = min(max(int(nlay[r]), 0), Lmax)
        junk = np.nan if r % 2 else 1e30
        h[r, max(n - 1, 0):] = junk                                              # the half-space's thickness too
        q[r, n:] = junk
        K[r, :, :, n:] = junk
    return dict(nlay=nlay, h=np.ascontiguousarray(h), q=np.ascontiguousarray(q), K=np.ascontiguousarray(K),
                c=np.ascontiguousarray(c), w=w)


def built_rows(Lmax=LMAX):
    """Thicknesses of the finite layers: one thick layer (a bin inside one layer, a layer over many bins, a stack that
    ends beyond the last edge), nlay = Lmax with interfaces on the coarse edges and a layer of thickness 0 (the stack
    ends at 23.75 km: inside the fine and the last coarse bins' range), a thin stack inside the first bin, interfaces at
    2, 3 and 5 km."""
    return [[70.], [5., 5., 10., 0., 2.5, 1., 0.25][:Lmax - 1], [0.3, 0.1], [2., 1., 2.]]


def rows_of(case, a, b):
    return {k: v[a:b] for k, v in case.items()}


def twin(ssim, case, start, edges, kind, weights=True, drho=0.32):
    """The host twin -> bh_sens_sets_finish's arrays."""
    start = np.ascontiguousarray(start, dtype=np.int64)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    Z, (R, nper, _, Lmax) = start.size - 1, case['K'].shape
    assert start[-1] == R
    out = dict(total=np.zeros((Z, nper), dtype=np.int64), excluded=np.zeros((Z, nper), dtype=np.int64))
    for k in FIELDS[2:]:
        out[k] = np.zeros((Z, nper, edges.size))
    arr = {k: np.ascontiguousarray(v) for k, v in case.items()}
    q = arr['q'] if kind == 'vs_total' else None
    rc = ssim.sss_sets(start.ctypes.data, Z, nper, edges.ctypes.data, edges.size, ref.KINDS[kind], drho, Lmax,
                       arr['h'].shape[1], arr['nlay'].ctypes.data, arr['h'].ctypes.data,
                       None if q is None else q.ctypes.data, 0 if q is None else q.shape[1], arr['K'].ctypes.data,
                       arr['c'].ctypes.data, arr['w'].ctypes.data if weights else None, *[out[k].ctypes.data for k in FIELDS])
    assert rc == 0
    return out


def errors_over_bounds(got, z, want, Lmax):
    """Set z of the sums `got` against the restatement `want` -> (worst |mean error| / bound, worst |variance error| /
    bound); counts and NaN patterns must agree."""
    assert np.array_equal(got['total'][z], want['total']) and np.array_equal(got['excluded'][z], want['excluded'])
    W = got['total'][z].astype(np.float64)[:, None]
    live = (want['total'] > 0)[:, None] & np.ones(got['s1'][z].shape, dtype=bool)
    assert np.array_equal(np.isnan(got['vmin'][z]), ~live) and np.array_equal(np.isnan(got['vmax'][z]), ~live)
    assert not got['s1'][z][~live].any() and not got['s2'][z][~live].any()
    if not live.any():
        return 0., 0.
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = got['s1'][z] / W
        var = got['s2'][z] / W - mean * mean
    worst = []
    for val, name, bound in ((mean, 'mean', tol.mean_bound(want['n'], Lmax, want['absmean'])),
                             (var, 'var', tol.var_bound(want['n'], Lmax, want['sqmean']))):
        err = np.abs(val[live].astype(np.longdouble) - want[name][live]).astype(np.float64)
        worst.append(float(np.where(err == 0, 0., err / np.where(err == 0, 1., bound[live])).max()))
    return tuple(worst)


def assert_same_bits(a, b):
    assert a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('grid', sorted(EDGES))
def test_twin_lies_within_the_bounds_of_the_restatement(ssim, grid, kind):
    case, edges = make_case(41, 300), EDGES[grid]
    assert case['nlay'].min() == 1 and case['nlay'].max() == LMAX + 1 and (case['w'] == 0).sum() > 10
    assert (case['nlay'] == 2).any() and (case['nlay'] == LMAX).any() and np.isnan(case['c']).sum() > 10
    sizes = [4, 1, 0, 295]                             # the built geometries alone, one row, none, all the rest
    start = np.concatenate(([0], np.cumsum(sizes)))
    got = twin(ssim, case, start, edges, kind)
    worst = [0., 0.]
    for z in range(len(sizes)):
        r = rows_of(case, start[z], start[z + 1])
        want = ref.summarize(r['nlay'], r['h'], r['q'], r['K'], r['c'], r['w'], edges, kind)
        e = errors_over_bounds(got, z, want, LMAX)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print('%s %s: worst error / bound: mean %.3g, variance %.3g' % (grid, kind, worst[0], worst[1]))
    assert worst[0] <= 1. and worst[1] <= 1., worst
    assert got['total'][2].sum() == 0 and got['excluded'][2].sum() == 0


def test_the_built_geometries_are_what_they_say(ssim):
    """By the restatement alone, on K = 1 for dc/dvs: a cell is then the fraction of its layers that falls into it."""
    case = make_case(42, 4)
    case['K'][:, :, 2, :] = 1.
    case['c'][:] = 3.
    x, model = ref.row_cells(case['nlay'], case['h'], None, case['K'], case['c'], EDGES['fine'], 'vs')
    assert model.all()
    x = x[:, 0, :-1].astype(np.float64)
    assert np.allclose(x[0], 0.5 / 70.)                                     # every bin inside the one layer
    assert np.isclose(x[1].sum(), 7. - 1.) and x[1][48:].sum() == 0        # the layer of thickness 0 adds nothing; ends at 23.75
    assert np.isclose(x[1][47], 1.0)                                        # 23.5 .. 23.75 is all of the last finite layer
    assert np.isclose(x[2][0], 2.) and not x[2][1:].any()                   # both thin layers lie in the first bin
    assert np.allclose(x[3][:4], 0.25) and np.allclose(x[3][4:6], 0.5) and np.allclose(x[3][6:10], 0.25)
    y, _ = ref.row_cells(case['nlay'], case['h'], None, case['K'], case['c'], EDGES['one'], 'vs')
    assert np.isclose(float(y[0, 0, 0]), 38.5 / 70.) and np.isclose(float(y[2, 0, 0]), 0.)     # what lies above 1.5 km is dropped
    z, _ = ref.row_cells(case['nlay'], case['h'], None, case['K'], case['c'], EDGES['coarse'], 'vs')
    assert np.allclose(z[3, 0, :-1].astype(np.float64), [1., 1., 0., 0., 0., 0.])           # interfaces on the edges: whole layers
    assert np.allclose(z[1, 0, :-1].astype(np.float64), [0.2, 0.4, 1., 1., 3., 0.])
    got = twin(ssim, case, [0, 4], EDGES['coarse'], 'vs')
    assert np.all(got['s1'][0][:, -1] == case['w'].sum())                                 # the half-space's K = 1


def test_min_and_max_are_exact_and_sets_equal_their_rows_alone(ssim):
    case, edges = make_case(43, 1300), EDGES['fine']
    sizes = [0, 1, 255, 256, 257, 513, 18]          # sets that start inside another set's would-be block
    start = np.concatenate(([0], np.cumsum(sizes)))
    case['w'][start[1]] = 2                         # the one-row set (a built row: it has a model) has weight
    case['w'][start[6]:] = 0                        # the last set: rows, no weight
    got = twin(ssim, case, start, edges, 'vs_total')
    for z, n in enumerate(sizes):
        a, b = start[z], start[z + 1]
        alone = twin(ssim, rows_of(case, a, b) if n else rows_of(case, 0, 1), [0, n] if n else [0, 0, 1], edges, 'vs_total')
        for k in FIELDS:
            assert_same_bits(got[k][z], alone[k][0])
    for z in (0, 6):
        assert not got['total'][z].any() and np.isnan(got['vmin'][z]).all() and not got['s1'][z].any()
    assert not got['excluded'][6].any()             # weight 0 is not excluded weight
    # every row as a set of its own with weight 1: s1 is then the row's cell, to the bit
    z = 5
    a, b = start[z], start[z + 1]
    one = twin(ssim, rows_of(case, a, b), np.arange(b - a + 1), edges, 'vs_total', weights=False)
    counts = (one['total'] > 0) & (case['w'][a:b] > 0)[:, None]                       # [rows, nper]
    assert np.array_equal(counts.sum(axis=0) > 0, got['total'][z] > 0)
    x = np.where(counts[:, :, None], one['s1'], np.nan)
    assert (got['total'][z] > 0).all()
    assert np.array_equal(np.nanmin(x, axis=0), got['vmin'][z]) and np.array_equal(np.nanmax(x, axis=0), got['vmax'][z])
    assert np.array_equal(one['vmin'][counts], one['s1'][counts]) and np.array_equal(one['vmax'][counts], one['s1'][counts])
    # without weights every row counts once
    plain = twin(ssim, case, start, edges, 'vs_total', weights=False)
    ones = dict(case, w=np.ones_like(case['w']))
    for k in FIELDS:
        assert_same_bits(plain[k], twin(ssim, ones, start, edges, 'vs_total')[k])


def test_bins_and_half_space_add_up_to_the_layers(ssim):
    """Edges that cover every stack (0 .. 80 km over at most 7 layers of at most 9 km): the sum over the cells of the
    mean is the mean over the rows of the sum over the layers, within the sum of the cells' bounds."""
    case = make_case(44, 200, built=False)
    edges = np.linspace(0., 80., 33)
    got = twin(ssim, case, [0, 200], edges, 'vs')
    want = ref.summarize(case['nlay'], case['h'], None, case['K'], case['c'], case['w'], edges, 'vs')
    assert max(errors_over_bounds(got, 0, want, LMAX)) <= 1.
    w, nlay = case['w'].astype(np.int64), case['nlay']
    model = (nlay >= 2) & (nlay <= LMAX)
    for p in range(5):
        rows = np.nonzero((w > 0) & model & ~np.isnan(case['c'][:, p]))[0]
        thick = lambda r: np.r_[case['h'][r, :nlay[r] - 1] > 0, True]             # a layer of thickness 0 is in no bin
        layers = sum(np.longdouble(w[r]) * case['K'][r, p, 2, :nlay[r]][thick(r)].astype(np.longdouble).sum() for r in rows)
        W = np.longdouble(w[rows].sum())
        cells = (got['s1'][0][p].astype(np.longdouble) / W).sum()
        bound = tol.mean_bound(want['n'], LMAX, want['absmean'])[p].sum()
        assert abs(float(cells - layers / W)) <= bound, (p, float(cells - layers / W), bound)


def test_from_sums_rules():
    from bayhunter_amd.sensitivity import from_sums
    total = np.array([10, 0, 3])
    s1 = np.array([[5., 1.], [0., 0.], [0.3, 0.9]])
    s2 = np.array([[4.5, 0.1], [0., 0.], [0.03000000000000001, 0.29]])
    vmin = np.array([[0.1, 0.1], [np.nan, np.nan], [0.1, 0.2]])
    vmax = np.array([[0.9, 0.1], [np.nan, np.nan], [0.1, 0.4]])
    mean, std = from_sums(total, s1, s2, vmin, vmax)
    assert np.array_equal(mean[0], [0.5, 0.1]) and std[0, 0] == np.sqrt(4.5 / 10 - 0.25)
    assert std[0, 1] == 0. and 0.1 / 10 - 0.1 * 0.1 != 0.           # vmin == vmax: exactly 0, whatever the sums say
    assert std[2, 0] == 0. and std[2, 1] == np.sqrt(max(0., 0.29 / 3 - (0.9 / 3) ** 2))
    assert np.isnan(mean[1]).all() and np.isnan(std[1]).all()        # a period without weight
    m, s = from_sums(np.array([4]), np.array([[2.]]), np.array([[0.999999]]), np.array([[0.4]]), np.array([[0.6]]))
    assert m[0, 0] == 0.5 and s[0, 0] == 0.                          # a variance rounded below 0 is 0
    stacked = from_sums(np.stack([total, total]), np.stack([s1, s1]), np.stack([s2, s2]), np.stack([vmin, vmin]),
                        np.stack([vmax, vmax]))
    assert np.array_equal(stacked[0][1], mean, equal_nan=True) and np.array_equal(stacked[1][0], std, equal_nan=True)


def test_split_runs_cuts_sets_at_block_multiples_only():
    from bayhunter_amd import _lib
    from bayhunter_amd.sensitivity import split_runs
    blk = _lib.SENS_SETS_BLOCK_ROWS
    start = np.array([0, 0, 100, 1000, 1000, 1300, 1301])
    for max_rows in (1, 100, 255, 256, 300, 512, 900, 1301, 5000):
        runs = split_runs(start, max_rows)
        assert runs[0][0] == 0 and runs[-1][1] == 1301 and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        for lo, hi in runs:
            assert hi > lo and (hi - lo <= max(max_rows, blk))
            for r in (lo, hi):
                z = np.searchsorted(start, r, side='right') - 1
                assert r in start or (r - start[z]) % blk == 0, (max_rows, runs)
    assert split_runs(start, 5000) == [(0, 1301)] and split_runs(start, 300) == [(0, 100), (100, 356), (356, 612), (612, 868),
                                                                              (868, 1000), (1000, 1300), (1300, 1301)]
    assert split_runs(np.array([0, 0]), 10) == []


def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    edges = EDGES['fine'].copy()

    def create(start=(0, 4, 10), nsets=2, nper=5, e=edges, ne=None, kind=4, drho=0.32):
        h = C.c_void_p(77)
        start = None if start is None else np.asarray(start, dtype=np.int64)
        rc = lib.bh_sens_sets_create(C.byref(h), None if start is None else start.ctypes.data, nsets, nper,
                                     None if e is None else e.ctypes.data, (0 if e is None else e.size) if ne is None else ne,
                                     kind, drho, None)
        if rc == _lib.BH_OK:
            lib.bh_sens_sets_destroy(h)
        else:
            assert not h.value                       # no handle comes back with an error
        return rc
    err = lambda: lib.bh_last_error()
    assert create(nsets=0) == E and b'sets' in err() and create(nsets=_lib.PAIRS_MAX_SETS + 1) == E
    assert create(start=None) == E and create(start=(1, 4, 10)) == E and b'begin at 0' in err()
    assert create(start=(0, 6, 4, 10), nsets=3) == E and b'ascending' in err()
    assert create(nper=0) == E and create(nper=_lib.MAX_PERIODS + 1) == E and b'nper' in err()
    assert create(e=None) == E and create(ne=1) == E and b'depth edges' in err()
    assert create(e=np.arange(_lib.SENS_SETS_MAX_BINS + 2.)) == E and b'depth edges' in err()
    assert create(e=edges[::-1].copy()) == E and b'ascending' in err()
    for v in (np.nan, np.inf, -np.inf):
        bad = edges.copy()
        bad[0 if v == -np.inf else -1] = v
        assert create(e=bad) == E and b'finite' in err()
    for kind in (0, 5, -1):                          # dc/dh (K's kind 0) is not offered
        assert create(kind=kind) == E and b'kind' in err()
    assert create(drho=np.nan) == E and b'drho_dvp' in err()
    assert create() in (_lib.BH_OK, _lib.BH_ERR_NO_DEVICE)          # everything was in order
    nodev = C.c_void_p(16)
    assert lib.bh_sens_sets_add(None, 0, 4, 8, 8, nodev, nodev, nodev, 8, nodev, nodev, None) == E and b'handle' in err()
    assert lib.bh_sens_sets_finish(None, None, None, None, None, None, None) == E and b'handle' in err()
    lib.bh_sens_sets_destroy(None)
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read()
    for name, v in _lib.SENS_KINDS.items():
        assert '#define BH_SENS_KIND_%-8s %d' % (name.upper(), v) in header
    assert '#define BH_SENS_SETS_BLOCK_ROWS %d' % _lib.SENS_SETS_BLOCK_ROWS in header
    assert '#define BH_SENS_SETS_MAX_BINS   %d' % _lib.SENS_SETS_MAX_BINS in header
    assert 'sens_sets.hip' in _lib.SOURCES and 'sens_sets_core.h' in _lib.HEADERS
    for f in ('create', 'add', 'finish', 'destroy'):
        assert 'bh_sens_sets_' + f in _lib.EXPORTS


def test_python_layer_refuses_bad_arguments():
    from bayhunter_amd import sensitivity as sens
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool, StationView
    rows, per = np.zeros((10, 4)), np.array([5., 10.])
    for start in ([0, 6, 4, 10], [0, 4, 9], [1, 10], [0]):
        with pytest.raises(ValueError, match='set_start'):
            sens.summarize_sets(per, 'rayleigh', rows, start, 1.73, device='cpu')
    with pytest.raises(ValueError, match='wave'):
        sens.summarize(per, 'stoneley', rows, 1.73, device='cpu')
    with pytest.raises(ValueError, match='kind'):
        sens.summarize(per, 'love', rows, 1.73, kind='h', device='cpu')
    with pytest.raises(ValueError, match='more than 60 periods'):
        sens.summarize(np.linspace(1., 40., 61), 'love', rows, 1.73, device='cpu')
    with pytest.raises(ValueError, match='periods'):
        sens.summarize([], 'love', rows, 1.73, device='cpu')
    with pytest.raises(ValueError, match='vpvs'):
        sens.summarize(per, 'love', rows, np.ones(9), device='cpu')
    with pytest.raises(ValueError, match='one weight per row'):
        sens.summarize(per, 'love', rows, 1.73, np.ones(9, dtype=np.int32), device='cpu')
    with pytest.raises(ValueError, match='negative weight'):
        sens.summarize(per, 'love', rows, 1.73, np.array([1] * 9 + [-1]), device='cpu')
    with pytest.raises(ValueError, match='max_rows'):
        sens.summarize(per, 'love', rows, 1.73, max_rows=0, device='cpu')
    for bad in ([0., 1., 1.], [2., 1.], [0.], [0., np.nan], [0., np.inf], np.arange(1026.)):
        with pytest.raises(ValueError, match='dep_edges'):
            sens.summarize(per, 'love', rows, 1.73, dep_edges=bad, device='cpu')
    with pytest.raises(ValueError, match='empty selection'):
        sens.summarize(per, 'love', np.zeros((0, 4)), 1.73, device='cpu')
    from bayhunter_amd import interfaces
    assert np.array_equal(sens.default_edges(), interfaces._edges(None, None)[0])
    assert callable(ChainPool.sensitivity) and callable(StationPool.sensitivity) and StationView.sensitivity is ChainPool.sensitivity
