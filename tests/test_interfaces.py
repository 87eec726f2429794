"""CPU tier of the discontinuity statistics (bayhunter_amd/interfaces.py, csrc/interfaces_core.h, csrc/interfaces.hip):

* the host twin (tests/hostsim/interfaces_sim.cpp: the kernels' per-row walk compiled with g++, the float sums in the
  kernels' order) equals the numpy restatement (tests/interfaces_ref.py) exactly on every integer field, in float32
  and float64: a random campaign and the built edge cases;
* its jump mean and standard deviation lie within the derived bound (tests/interfaces_tolerances.py) of the
  restatement's longdouble moments;
* one model worked by hand;
* many sets in one call equal the per-set calls bit for bit, and taking the depth bins in groups changes no count;
* bh_interfaces_sets and the Python layer refuse bad arguments before they touch a device.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import interfaces_ref as ref  # noqa: E402
import interfaces_tolerances as tol  # noqa: E402

WIDTH = 42                                   # n = 1 .. 21
DEDGES = np.arange(0., 61., 5.)              # 12 depth bins, the last edge 60 km
JEDGES = np.linspace(-2., 2., 9)             # 8 jump bins of 0.5 km/s
FP = ('jsum', 'jsq')


def load_sim():
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so = os.path.join(d, 'libinterfaces_sim.so')
    srcs = [os.path.join(d, 'interfaces_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                      ('interfaces_core.h', 'posterior_core.h', 'stats_core.h', 'bh_common.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so, srcs[0]], check=True)
    lib = C.CDLL(so)
    for f in (lib.ifs_sets32, lib.ifs_sets64):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                      C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.ifs_blocks_of.argtypes = [C.c_longlong]
    return lib


@pytest.fixture(scope='module')
def isim():
    return load_sim()


def twin(isim, rows, weights=None, set_start=None, dedges=DEDGES, jedges=JEDGES, group=0):
    """The host twin on `rows` -> the dict of arrays with one row per set that interfaces._reduce returns."""
    rows = np.ascontiguousarray(rows)
    R = rows.shape[0]
    start = np.array([0, R] if set_start is None else set_start, dtype=np.int64)
    S, nbd, nbj = start.size - 1, dedges.size - 1, jedges.size - 1
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
    total = np.zeros(S, dtype=np.int64)
    fields = np.zeros((6, S, nbd), dtype=np.int64)
    hist = np.zeros((S, nbd, nbj), dtype=np.int64)
    jsum, jsq = np.zeros((S, nbd)), np.zeros((S, nbd))
    dedges, jedges = np.ascontiguousarray(dedges, dtype=np.float64), np.ascontiguousarray(jedges, dtype=np.float64)
    fn = isim.ifs_sets64 if rows.dtype == np.float64 else isim.ifs_sets32
    rc = fn(rows.ctypes.data, R, rows.shape[1], rows.shape[1], None if w is None else w.ctypes.data, start.ctypes.data,
            S, dedges.ctypes.data, dedges.size, jedges.ctypes.data, jedges.size, group, total.ctypes.data,
            fields.ctypes.data, hist.ctypes.data, jsum.ctypes.data, jsq.ctypes.data)
    assert rc == 0
    res = dict(total=total, hist=hist, jsum=jsum, jsq=jsq)
    res.update({k: fields[i] for i, k in enumerate(ref.COUNTS)})
    return res


def assert_counts(res, z, want, what=''):
    assert int(res['total'][z]) == want['total'], what
    for k in ref.COUNTS + ('hist',):
        assert res[k][z].dtype == np.int64 and np.array_equal(res[k][z], want[k]), (what, k, res[k][z], want[k])


def moment_errors(got, want):
    """The jump mean / std of summarize()'s dict `got` against the restatement `want` -> (worst |error| / bound of the
    mean, of the std); the NaN patterns must agree."""
    cnt = want['count']
    worst = []
    for name, bound in (('jump_mean', tol.mean_bound(want['addends'], want['absum'], cnt, want['jump_mean'])),
                        ('jump_std', tol.std_bound(want['addends'], want['absum'], cnt, want['jump_mean'], want['jump_std']))):
        assert np.array_equal(np.isnan(got[name]), cnt == 0), name
        live = cnt > 0
        err = np.abs(got[name][live].astype(np.longdouble) - want[name][live]).astype(np.float64)
        ratio = np.where(err == 0, 0., err / bound[live])
        worst.append(float(ratio.max()) if live.any() else 0.)
    return tuple(worst)


def built_cases(dtype):
    """(rows, weights, names): one row per edge case, on DEDGES / JEDGES."""
    L = lambda vs, ifs: ref.layered_row(vs, ifs, WIDTH, dtype)
    cases = [
        ('one nucleus', L([3.3], []), 2),
        ('n = maxlayers', L(np.linspace(2., 4.5, 21) + 0.3 * (np.arange(21) % 3 == 1), np.linspace(2., 58., 20)), 3),
        ('all NaN', np.full(WIDTH, np.nan).astype(dtype), 4),
        ('weight 0', L([3., 4.], [22.]), 0),
        ('interface on an inner edge', L([3., 3.25], [10.]), 1),
        ('interface on the last edge', L([3., 3.25], [60.]), 2),
        ('jump on a jump edge', L([3., 3.5], [33.]), 1),
        ('jump of zero', L([3.5, 3.5], [41.]), 5),
        ('two in one bin', L([3., 3.25, 3.75], [11., 12.]), 2),
        ('three in one bin', L([3., 3.25, 3.75, 4.], [46., 47., 48.]), 3),
        ('two in one bin, mixed signs', L([3., 3.75, 3.25], [26., 27.]), 2),
        ('three in one bin, mixed signs', L([3., 2.5, 3.25, 2.75], [51., 52., 53.]), 1),
        ('jump outside the jump edges', L([1., 4.5, 1.25], [16., 36.]), 2),
        ('interface outside the depth edges', L([3., 3.25, 3.5], [57., 70.]), 3),
    ]
    names = [c[0] for c in cases]
    return np.stack([c[1] for c in cases]), np.array([c[2] for c in cases], dtype=np.int32), names


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_twin_equals_the_restatement_on_a_random_campaign(isim, dtype):
    rs = np.random.RandomState(21 if dtype == np.float32 else 22)
    rows = ref.random_rows(rs, 4000, WIDTH, dtype)
    w = rs.randint(0, 6, 4000).astype(np.int32)
    n = (~np.isnan(rows)).sum(axis=1) // 2
    assert n.min() == 0 and n.max() == 21 and (w == 0).sum() > 100
    want = ref.summarize(rows, w, DEDGES, JEDGES)
    assert (want['models'] < want['count']).all() and want['neg'].min() > 0 and want['pos'].min() > 0    # by the restatement alone
    assert want['hist'].sum() < want['count'].sum()                                     # some jumps lie outside
    res = twin(isim, rows, w)
    assert_counts(res, 0, want)
    # depth bins in groups, as the kernel takes them when its LDS is short: the same counts
    for group in (1, 5, 7):
        assert_counts(twin(isim, rows, w, group=group), 0, want, 'group %d' % group)
    from bayhunter_amd import interfaces
    got = interfaces._result(res, 0, DEDGES, JEDGES)
    worst = moment_errors(got, want)
    print('worst error / bound: jump_mean %.3g, jump_std %.3g' % worst)
    assert worst[0] <= 1. and worst[1] <= 1., worst
    assert np.array_equal(got['p_interface'], want['models'] / float(want['total']))
    assert np.array_equal(got['p_neg'], want['models_neg'] / float(want['total']))
    assert np.array_equal(got['p_pos'], want['models_pos'] / float(want['total']))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_twin_equals_the_restatement_on_the_built_cases(isim, dtype):
    rows, w, names = built_cases(dtype)
    wants = {}
    for i, name in enumerate(names):                # each case alone, then all together
        wants[name] = want = ref.summarize(rows[i:i + 1], w[i:i + 1], DEDGES, JEDGES)
        res = twin(isim, rows[i:i + 1], w[i:i + 1])
        assert_counts(res, 0, want, name)
    want = ref.summarize(rows, w, DEDGES, JEDGES)
    res = twin(isim, rows, w)
    assert_counts(res, 0, want, 'all')
    from bayhunter_amd import interfaces
    worst = moment_errors(interfaces._result(res, 0, DEDGES, JEDGES), want)
    assert worst[0] <= 1. and worst[1] <= 1., worst
    # the cases are what their names say, by the restatement
    c = lambda name, field: wants[name][field]
    for name in ('one nucleus', 'all NaN'):
        assert c(name, 'total') > 0 and c(name, 'count').sum() == 0 and c(name, 'models').sum() == 0
    assert c('weight 0', 'total') == 0 and c('weight 0', 'count').sum() == 0
    assert c('n = maxlayers', 'count').sum() == 20 * 3 and (~np.isnan(rows[names.index('n = maxlayers')])).sum() == WIDTH
    assert c('interface on an inner edge', 'count')[2] == 1 and c('interface on an inner edge', 'count').sum() == 1
    assert c('interface on the last edge', 'count')[-1] == 2                          # closed on the right
    assert c('jump on a jump edge', 'hist')[6, 5] == 1 and JEDGES[5] == 0.5           # 0.5 opens its bin
    z = wants['jump of zero']
    assert z['count'][8] == 5 and z['neg'].sum() == 0 and z['pos'].sum() == 0 and z['models_neg'].sum() == 0
    assert z['hist'][8, 4] == 5 and JEDGES[4] == 0.
    assert c('two in one bin', 'count')[2] == 4 and c('two in one bin', 'models')[2] == 2
    assert c('three in one bin', 'count')[9] == 9 and c('three in one bin', 'models')[9] == 3
    assert c('three in one bin', 'models_pos')[9] == 3 and c('three in one bin', 'pos')[9] == 9
    m = wants['two in one bin, mixed signs']
    assert (m['count'][5], m['models'][5], m['neg'][5], m['pos'][5], m['models_neg'][5], m['models_pos'][5]) == (4, 2, 2, 2, 2, 2)
    m = wants['three in one bin, mixed signs']
    assert (m['count'][10], m['models'][10], m['neg'][10], m['pos'][10], m['models_neg'][10], m['models_pos'][10]) == (3, 1, 2, 1, 1, 1)
    o = wants['jump outside the jump edges']
    assert o['count'].sum() == 4 and o['hist'].sum() == 0 and o['pos'][3] == 2 and o['neg'][7] == 2
    o = wants['interface outside the depth edges']
    assert o['count'].sum() == 3 and o['count'][11] == 3 and o['total'] == 3


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_model_worked_by_hand(isim, dtype):
    # interfaces at 10 and 30 km, Vs 3.0 / 3.5 / 3.25, held for two iterations; a half-space held for three
    rows = np.stack([ref.layered_row([3.0, 3.5, 3.25], [10., 30.], 8, dtype), ref.layered_row([4.0], [], 8, dtype)])
    w = np.array([2, 3], dtype=np.int32)
    dedges, jedges = np.array([0., 20., 40.]), np.array([-1., 0., 1.])
    res = twin(isim, rows, w, dedges=dedges, jedges=jedges)
    from bayhunter_amd import interfaces
    got = interfaces._result(res, 0, dedges, jedges)
    assert got['total'] == 5
    for k, hand in (('count', [2, 2]), ('models', [2, 2]), ('pos', [2, 0]), ('neg', [0, 2]), ('models_pos', [2, 0]),
                    ('models_neg', [0, 2])):
        assert got[k].tolist() == hand, k
    assert got['hist'].tolist() == [[0, 2], [2, 0]]
    assert got['jsum'].tolist() == [1.0, -0.5] and got['jsq'].tolist() == [0., 0.]
    assert got['jump_mean'].tolist() == [0.5, -0.25] and got['jump_std'].tolist() == [0., 0.]
    assert got['p_interface'].tolist() == [0.4, 0.4] and got['p_pos'].tolist() == [0.4, 0.] and got['p_neg'].tolist() == [0., 0.4]
    assert_counts(res, 0, ref.summarize(rows, w, dedges, jedges))


def assert_same_bits(a, b):
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_sets_equal_the_per_set_calls(isim, dtype):
    rs = np.random.RandomState(23)
    per_block = isim.ifs_rows_per_block()
    sizes = [0, 1, 255, 0, per_block + 3, 40]       # an empty set first and inside, one row, more than one block
    start = np.concatenate(([0], np.cumsum(sizes)))
    assert [isim.ifs_blocks_of(s) for s in sizes] == [0, 1, 1, 0, 2, 1]
    rows = ref.random_rows(rs, start[-1], WIDTH, dtype)
    w = rs.randint(0, 4, start[-1]).astype(np.int32)
    w[start[5]:] = 0                                # the last set: rows, but no weight
    w[0] = 2                                        # the one-row set
    res = twin(isim, rows, w, start)
    for z, n in enumerate(sizes):
        a, b = start[z], start[z + 1]
        if n:
            one = twin(isim, rows[a:b], w[a:b])
            assert_counts(res, z, ref.summarize(rows[a:b], w[a:b], DEDGES, JEDGES), 'set %d' % z)
        else:
            one = twin(isim, rows[:1], np.zeros(1, dtype=np.int32))
        for k in ('total', 'hist') + ref.COUNTS:
            assert np.array_equal(res[k][z], one[k][0]), (z, k)
        for k in FP:
            assert_same_bits(res[k][z], one[k][0])
        if z in (0, 3, 5):                          # empty, or without weight: counts 0, float fields NaN
            assert res['total'][z] == 0 and not res['count'][z].any() and np.isnan(res['jsum'][z]).all() and np.isnan(res['jsq'][z]).all()
    from bayhunter_amd import interfaces
    assert interfaces._result(res, 0, DEDGES, JEDGES) is None and interfaces._result(res, 1, DEDGES, JEDGES)['total'] == w[0]


@pytest.fixture(scope='module')
def nodev():
    return C.c_void_p(16)                  # never dereferenced: the arguments are checked first


def test_capi_refuses_bad_arguments(lib, nodev):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    de, je = DEDGES.copy(), JEDGES.copy()
    out = np.zeros((2, 12, 8), dtype=np.int64)
    fp = np.zeros((2, 12))

    def call(rows=nodev, nrows=10, stride=42, width=42, start=(0, 4, 10), nsets=2, dedges=de, nde=None, jedges=je,
             nje=None, hist=out):
        start = None if start is None else np.asarray(start, dtype=np.int64)
        p = lambda a: None if a is None else a.ctypes.data
        return lib.bh_interfaces_sets(rows, 0, nrows, stride, width, None, p(start), nsets, p(dedges),
                                      (0 if dedges is None else dedges.size) if nde is None else nde, p(jedges),
                                      (0 if jedges is None else jedges.size) if nje is None else nje, p(out), p(out), p(out),
                                      p(out), p(out), p(out), p(out), p(hist), p(fp), p(fp), None)
    err = lambda: lib.bh_last_error()
    assert call(rows=None) == E and b'no rows' in err()
    assert call(nrows=0, start=(0, 0, 0)) == E and b'no rows' in err()
    assert call(nrows=(1 << 32) + 1, start=(0, 4, (1 << 32) + 1)) == E and b'2^32' in err()
    assert call(stride=41) == E and b'stride' in err()
    assert call(width=1, stride=42) == E and call(width=400, stride=400) == E and b'width' in err()
    assert call(nsets=0) == E and b'sets' in err()
    assert call(nsets=_lib.PAIRS_MAX_SETS + 1) == E
    assert call(start=None) == E
    assert call(start=(0, 6, 4, 10), nsets=3) == E and b'ascending' in err()
    assert call(start=(0, 4, 9)) == E and b'end at nrows' in err()
    assert call(start=(1, 4, 10)) == E
    assert call(dedges=None) == E and b'depth edges' in err()
    assert call(nde=1) == E and call(dedges=np.arange(_lib.INTERFACES_MAX_DEPTH_BINS + 2.)) == E
    assert call(dedges=de[::-1].copy()) == E and b'ascending' in err()
    bad = de.copy()
    bad[3] = bad[2]
    assert call(dedges=bad) == E and b'depth edges' in err()
    for v in (np.nan, np.inf, -np.inf):
        bad = de.copy()
        bad[0 if v == -np.inf else -1] = v
        assert call(dedges=bad) == E and b'finite' in err()
        bad = je.copy()
        bad[0 if v == -np.inf else -1] = v
        assert call(jedges=bad) == E and b'jump edges' in err()
    assert call(jedges=je[::-1].copy()) == E and b'jump edges' in err()
    assert call(nje=1) == E and call(jedges=np.arange(_lib.INTERFACES_MAX_JUMP_BINS + 2.)) == E
    assert call(jedges=None) == E and b'hist needs' in err()
    # the limits are the header's
    assert _lib.INTERFACES_MAX_DEPTH_BINS >= 400 and _lib.INTERFACES_MAX_JUMP_BINS >= 64
    header = open(os.path.join(ROOT, 'include', 'bayhunter_amd.h')).read()
    assert '#define BH_INTERFACES_MAX_DEPTH_BINS %d' % _lib.INTERFACES_MAX_DEPTH_BINS in header
    assert '#define BH_INTERFACES_MAX_JUMP_BINS  %d' % _lib.INTERFACES_MAX_JUMP_BINS in header
    assert 'interfaces.hip' in _lib.SOURCES and 'interfaces_core.h' in _lib.HEADERS and 'bh_interfaces_sets' in _lib.EXPORTS


def test_python_layer_refuses_bad_arguments():
    from bayhunter_amd import interfaces
    rows = np.zeros((10, 4))
    for start in ([0, 6, 4, 10], [0, 4, 9], [1, 10], [0]):
        with pytest.raises(ValueError, match='set_start'):
            interfaces.summarize_sets(rows, start, device='cpu')
    with pytest.raises(ValueError, match='empty selection'):
        interfaces.summarize(np.zeros((0, 4)), device='cpu')
    with pytest.raises(ValueError, match='columns'):
        interfaces.summarize(np.zeros((10, 1)), device='cpu')
    with pytest.raises(ValueError, match='columns'):
        interfaces.summarize(np.zeros((10, 400)), device='cpu')
    with pytest.raises(ValueError, match='one weight per row'):
        interfaces.summarize(rows, np.ones(9, dtype=np.int32), device='cpu')
    with pytest.raises(ValueError, match='negative weight'):
        interfaces.summarize(rows, np.array([1] * 9 + [-1]), device='cpu')
    for bad in ([0., 1., 1.], [2., 1.], [0.], [0., np.nan], [0., np.inf], np.arange(1026.)):
        with pytest.raises(ValueError, match='dep_edges'):
            interfaces.summarize(rows, dep_edges=bad, device='cpu')
    for bad in ([0., 1., 1.], [2., 1.], [0.], [-np.inf, 0.], np.arange(258.)):
        with pytest.raises(ValueError, match='jump_edges'):
            interfaces.summarize(rows, jump_edges=bad, device='cpu')
    from bayhunter_amd import posterior
    de, je = interfaces._edges(None, None)
    assert np.array_equal(de, posterior.hist_grids(None)[1]) and np.array_equal(je, np.linspace(-2, 2, 41))
    from bayhunter_amd.chains import ChainPool
    from bayhunter_amd.stations import StationPool, StationView
    assert callable(ChainPool.interfaces) and callable(StationPool.interfaces) and StationView.interfaces is ChainPool.interfaces
