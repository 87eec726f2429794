"""CPU tier of the scalar-parameter posterior (bayhunter_amd/scalars.py, csrc/pairs_core.h, csrc/pairs.hip):

* the core of the segmented joint histograms, compiled with g++, gives the numpy restatement's counts
  (tests/scalars_ref.py: np.histogram2d on the expanded rows) exactly: a random campaign and the built edge cases,
  whatever the grouping of the pairs and the split of a set over blocks;
* the Python-side rules (median, edges, names) give numpy's own results, without a device;
* bh_hist2d_sets refuses bad arguments before it touches a device;
* the kernel of pairs.hip uses no scratch and its LDS stays within 64 KiB at 16 pairs x 64 bins.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import scalars_ref as ref  # noqa: E402


@pytest.fixture(scope='module')
def psim():
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so = os.path.join(d, 'libpairs_sim.so')
    srcs = [os.path.join(d, 'pairs_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h)
                                                 for h in ('pairs_core.h', 'stats_core.h', 'bh_common.h')]
    srcs.append(os.path.join(ROOT, 'include', 'bayhunter_amd.h'))
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so, srcs[0]],
                       check=True)
    lib = C.CDLL(so)
    lib.ps_plan.restype = C.c_long
    lib.ps_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.ps_hist2d_sets.restype = C.c_int
    lib.ps_hist2d_sets.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong]
    return lib


def sim(psim, D, weights, set_start, pairs, edges, group=0, rows_per_block=4096):
    D = np.ascontiguousarray(D, dtype=np.float64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
    start = np.ascontiguousarray(set_start, dtype=np.int64)
    pr = np.ascontiguousarray(pairs, dtype=np.int32)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    nb = edges.shape[2] - 1
    hist = np.full((start.size - 1, len(pairs), nb, nb), -1, dtype=np.int64)
    rc = psim.ps_hist2d_sets(D.ctypes.data, D.shape[0], D.shape[1], D.shape[1], None if w is None else w.ctypes.data,
                             start.ctypes.data, start.size - 1, pr.ctypes.data, len(pairs), edges.ctypes.data,
                             edges.shape[2], hist.ctypes.data, group, rows_per_block)
    assert rc == 0
    return hist


def set_edges(D, weights, set_start, nb):
    """Per set and column np.histogram's edges over the set's finite values of positive weight (anything ascending for
    a column without)."""
    S, K = len(set_start) - 1, D.shape[1]
    w = np.ones(D.shape[0], dtype=np.int64) if weights is None else np.asarray(weights)
    edges = np.zeros((S, K, nb + 1))
    edges[:] = np.arange(nb + 1)
    for s in range(S):
        for c in range(K):
            v = D[set_start[s]:set_start[s + 1], c][w[set_start[s]:set_start[s + 1]] > 0]
            v = v[~np.isnan(v)]
            if v.size:
                edges[s, c] = np.histogram(v, bins=nb)[1]
    return edges


def test_core_gives_the_restatements_counts_on_a_random_campaign(psim):
    rs = np.random.RandomState(21)
    sizes = [0, 1, 5000, 63, 9000, 257, 5674]                     # 19 995 rows in 7 sets
    start = np.concatenate(([0], np.cumsum(sizes)))
    R, K = start[-1], 6
    D = rs.randn(R, K) * np.array([1., 3., .1, 10., 1., 2.]) + np.arange(K)
    D[:, 4] = np.round(D[:, 4])                                   # a column of few distinct values: values on edges
    for c in range(K):
        D[rs.rand(R) < 0.03, c] = np.nan                          # per column independently
    w = rs.randint(0, 6, R).astype(np.int32)
    pairs = [(0, 1), (1, 0), (2, 2), (3, 4), (4, 5), (5, 0)]
    for nb in (1, 7, 50, 64):
        edges = set_edges(D, w, start, nb)
        edges[2, 3] = np.linspace(0., 12., nb + 1)                # edges that leave values outside on both sides
        want = ref.hist2d_sets(D, w, start, pairs, edges)
        assert want[0].sum() == 0 and want[2].sum() > 10000 and want[2, 3].sum() < want[2, 4].sum()
        assert np.array_equal(sim(psim, D, w, start, pairs, edges), want)
        # neither the grouping of the pairs nor the split of a set over blocks changes a count
        assert np.array_equal(sim(psim, D, w, start, pairs, edges, group=1, rows_per_block=100), want)
        assert np.array_equal(sim(psim, D, w, start, pairs, edges, group=4, rows_per_block=4097), want)
    assert np.array_equal(sim(psim, D, None, start, pairs, edges), ref.hist2d_sets(D, None, start, pairs, edges))


def built_cases():
    """One set per case: (name, rows [n, 2], weights, edges x, edges y)."""
    e = np.array([0., 1., 2., 4.])
    below, above = np.nextafter(e[0], -np.inf), np.nextafter(e[-1], np.inf)
    return [
        ('empty set', np.zeros((0, 2)), [], e, e),
        ('one row', [[0.5, 2.5]], [3], e, e),
        ('first edge', [[0., 0.]], [1], e, e),
        ('interior edge', [[1., 2.]], [1], e, e),
        ('last edge', [[4., 4.]], [1], e, e),
        ('one ulp below the first edge', [[below, 1.5], [1.5, below]], [1, 1], e, e),
        ('one ulp above the last edge', [[above, 1.5], [1.5, above]], [1, 1], e, e),
        ('NaN in x only', [[np.nan, 1.5]], [2], e, e),
        ('NaN in y only', [[1.5, np.nan]], [2], e, e),
        ('weight 0', [[1.5, 1.5], [0.5, 0.5]], [0, 4], e, e),
        ('eight weights of 2^30', [[1.5, 3.]] * 8, [1 << 30] * 8, e, e),
        ('constant column', [[7., 0.5]] * 3, [1, 2, 3], np.histogram(np.full(3, 7.), bins=3)[1], e),
    ]


def test_core_gives_the_restatements_counts_on_the_built_cases(psim):
    cases = built_cases()
    names = [c[0] for c in cases]
    D = np.concatenate([np.asarray(c[1], dtype=np.float64).reshape(-1, 2) for c in cases])
    w = np.concatenate([np.asarray(c[2], dtype=np.int32) for c in cases])
    start = np.concatenate(([0], np.cumsum([len(c[2]) for c in cases])))
    edges = np.stack([np.stack((c[3], c[4])) for c in cases])
    pairs = [(0, 1), (1, 0), (0, 0), (1, 1)]                      # cx == cy: the diagonal
    want = ref.hist2d_sets(D, w, start, pairs, edges)
    got = sim(psim, D, w, start, pairs, edges)
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), name
    assert np.array_equal(sim(psim, D, w, start, pairs, edges, group=1, rows_per_block=3), want)
    # the cases are what their names say, by the restatement
    h = dict(zip(names, want))
    cell = lambda name, p=0: [tuple(int(i) for i in ix) + (int(h[name][p][tuple(ix)]),) for ix in np.argwhere(h[name][p])]
    assert h['empty set'].sum() == 0
    assert cell('one row') == [(0, 2, 3)] and cell('one row', 1) == [(2, 0, 3)]
    assert cell('first edge') == [(0, 0, 1)] and cell('interior edge') == [(1, 2, 1)] and cell('last edge') == [(2, 2, 1)]
    for name in ('one ulp below the first edge', 'one ulp above the last edge'):
        assert h[name][0].sum() == 0 and h[name][1].sum() == 0
        assert cell(name, 2) == [(1, 1, 1)] and cell(name, 3) == [(1, 1, 1)]        # the other value of each row counts
    assert h['NaN in x only'][:3].sum() == 0 and cell('NaN in x only', 3) == [(1, 1, 2)]     # out of the pairs that read x
    assert h['NaN in y only'][[0, 1, 3]].sum() == 0 and cell('NaN in y only', 2) == [(1, 1, 2)]
    assert cell('weight 0') == [(0, 0, 4)]
    assert cell('eight weights of 2^30') == [(1, 2, 1 << 33)]
    e = edges[names.index('constant column'), 0]
    assert e[0] == 6.5 and e[-1] == 7.5 and cell('constant column') == [(1, 0, 6)]
    assert all(np.array_equal(h[n][2], np.diag(np.diag(h[n][2]))) for n in names)


def test_one_bin(psim):
    D = np.array([[0., 5.], [1., 6.], [2., 5.5], [np.nan, 5.]])
    edges = np.array([[[0., 2.], [5., 6.]]])
    want = ref.hist2d_sets(D, [1, 2, 3, 4], [0, 4], [(0, 1)], edges)
    assert want.shape == (1, 1, 1, 1) and want[0, 0, 0, 0] == 6
    assert np.array_equal(sim(psim, D, [1, 2, 3, 4], [0, 4], [(0, 1)], edges), want)


def test_the_lds_plan(psim):
    """Edges and cell tables stay within 64 KiB for every shape the entry point takes, one pair at least in a group."""
    from bayhunter_amd import _lib
    static = psim.ps_static_lds()
    for npairs in (1, 4, _lib.PAIRS_MAX):
        for ne in (2, 4, 21, 51, _lib.PAIRS_MAX_EDGES):
            for nslots in (1, min(2 * npairs, 3), 2 * npairs):
                g = C.c_int(0)
                dyn = psim.ps_plan(nslots, ne, npairs, C.byref(g))
                assert 1 <= g.value <= npairs and static + dyn <= 64 * 1024, (npairs, ne, nslots, g.value, dyn)
                assert dyn == 8 * nslots * ne + g.value * (ne - 1) ** 2 * 8
    g = C.c_int(0)
    psim.ps_plan(32, 65, 16, C.byref(g))
    assert g.value == 1                                            # 16 pairs x 64 bins: the pairs one after the other
    psim.ps_plan(4, 51, 3, C.byref(g))
    assert g.value == 3                                            # the Moho trade-off at 50 bins: one trip


# ---- the Python-side rules --------------------------------------------------------------------------------

def test_names():
    from bayhunter_amd import scalars
    assert scalars.NAMES(1, ['rdispph']) == ['like', 'misfit:rdispph', 'misfit:joint', 'vpvs', 'corr:rdispph',
                                             'sigma:rdispph', 'nlayers']
    assert scalars.NAMES(2, ['rdispph', 'prf'], moho=True) == [
        'like', 'misfit:rdispph', 'misfit:prf', 'misfit:joint', 'vpvs', 'corr:rdispph', 'sigma:rdispph', 'corr:prf',
        'sigma:prf', 'nlayers', 'moho']
    for nt in (1, 2):
        refs = ['t%d' % i for i in range(nt)]
        for moho in (False, True):
            assert len(scalars.TAGS(nt, moho)) == len(scalars.NAMES(nt, refs, moho)) == 3 * nt + 4 + moho
            tags = dict(zip(scalars.NAMES(nt, refs, moho), scalars.TAGS(nt, moho)))
            assert tags['like'] == tags['vpvs'] == 'f4' and tags['nlayers'] == 'n' and tags.get('moho', 'pair') == 'pair'
            assert all(t == 'f8' for n, t in tags.items() if n.split(':')[0] in ('misfit', 'corr', 'sigma'))
    with pytest.raises(ValueError):
        scalars.NAMES(2, ['a'])


@pytest.mark.parametrize('tag', ['f4', 'f8'])
def test_the_median_rule_is_np_median(tag):
    from bayhunter_amd import scalars
    rs = np.random.RandomState(5)
    dt = ref.DTYPE[tag]
    differs = 0
    for n in (1, 2, 3, 4, 7, 10, 101, 1000):
        for _ in range(20):
            v = (rs.randn(n) * 3 + 100).astype(dt)
            w = rs.randint(1, 4, n)
            full = np.sort(np.repeat(v, w))
            W = full.size
            lo, hi = np.float64(full[(W - 1) // 2]), np.float64(full[W // 2])
            got = scalars.median_of(lo, hi, W, tag)
            assert got.dtype == np.float64 and got == np.float64(np.median(np.repeat(v, w))), (n, W)
            differs += got != (lo + hi) / 2.
    assert (differs > 0) == (tag == 'f4')             # the float32 mean of two values is not their double mean


def test_the_edge_rules_are_np_histograms():
    from bayhunter_amd import scalars
    rs = np.random.RandomState(6)
    for tag in ('f4', 'f8'):
        for nbins in (1, 20, 33):
            v = (rs.randn(500) * 7 - 300).astype(ref.DTYPE[tag])
            want = np.histogram(v, bins=nbins)[1]
            got = scalars.column_edges(np.float64(v.min()), np.float64(v.max()), tag, nbins)
            assert got.dtype == want.dtype == ref.DTYPE[tag] and np.array_equal(got, want)
        v = np.full(9, 2.3, dtype=ref.DTYPE[tag])                 # a constant column
        want = ref.column(v, tag, 20)
        got = scalars.column_edges(2.3 if tag == 'f8' else np.float64(np.float32(2.3)), np.float64(v[0]), tag, 20)
        assert want['constant'] and got.dtype == want['hist'][1].dtype and np.array_equal(got, want['hist'][1])
        assert list(want['hist'][0]) == [0, 9, 0] and scalars.mode_of(want['hist'][0], got) == want['mode']
    layers = np.array([3., 5., 4., 4., 9.])
    want = ref.column(layers, 'n', 20)['hist']
    got = scalars.column_edges(3., 9., 'n', 20)
    assert np.array_equal(got, want[1]) and np.array_equal(got, np.arange(3, 11) - 0.5) and want[0].sum() == 5
    assert np.array_equal(scalars.column_edges(4., 4., 'n', 20), [3.5, 4.5])     # one layer count: one bin


def test_padded_edges_fold_back():
    """A finish over edges filled up to a common length: the padding's first bin holds the values on the last true
    edge, which np.histogram counts in its closed last bin."""
    from bayhunter_amd import scalars
    v = np.array([1., 2., 2.5, 4., 4.])
    e = np.histogram(v, bins=3)[1]
    p = scalars.padded_edges(e, 7)
    assert p.size == 7 and np.array_equal(p[:4], e) and np.all(np.diff(p) > 0)
    wide = np.histogram(v, bins=p)[0]
    assert wide[3] == 2                                           # the two values on the last edge
    assert np.array_equal(scalars.unpadded_hist(wide, 3), np.histogram(v, bins=3)[0])
    assert np.array_equal(scalars.unpadded_hist(np.histogram(v, bins=e)[0], 3), np.histogram(v, bins=3)[0])
    assert np.all(np.diff(scalars.padded_edges([-1e300, -5e299], 5)) > 0) and np.all(np.diff(scalars.padded_edges([0., 0.5], 4)) > 0)


def test_columns_and_pairs_are_checked():
    from bayhunter_amd import scalars
    data = np.zeros((4, 3))
    cols = scalars.Columns(data, ['f4', 'n', 'pair'], ['a', 'b', 'm'])
    assert cols.nstat == 2 and cols.index('m') == 2 and cols.index(1) == 1
    for bad in (dict(tags=['f4', 'pair', 'f8']), dict(tags=['pair'] * 3), dict(tags=['f4', 'f8']), dict(tags=['f4', 'x', 'f8']),
                dict(tags=['f4'] * 3, names=['a', 'a', 'b'])):
        with pytest.raises(ValueError):
            scalars.Columns(data, **bad)
    with pytest.raises(ValueError, match='no column'):
        scalars.summarize(cols, pairs=[('a', 'z')], device='cpu')
    with pytest.raises(ValueError, match='pair_bins'):
        scalars.summarize(cols, pairs=[('a', 'm')], pair_bins=65, device='cpu')
    with pytest.raises(ValueError, match='at most'):
        scalars.summarize(cols, pairs=[('a', 'm')] * 17, device='cpu')
    with pytest.raises(ValueError, match='nbins'):
        scalars.summarize(cols, nbins=0, device='cpu')


# ---- the library ------------------------------------------------------------------------------------------

def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    nodev = C.c_void_p(16)                  # never dereferenced: the arguments are checked first
    edges = np.tile(np.linspace(0., 1., 6), (2, 5, 1))
    hist = np.zeros((2, 2, 5, 5), dtype=np.int64)

    def call(D=nodev, nrows=10, stride=5, ncols=5, start=(0, 4, 10), nsets=2, pairs=((0, 1), (2, 3)), npairs=None,
             edges=edges, ne=6, hist=hist):
        st = None if start is None else np.asarray(start, dtype=np.int64)
        pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
        return lib.bh_hist2d_sets(D, nrows, stride, ncols, None, None if st is None else st.ctypes.data, nsets,
                                  None if pr is None else pr.ctypes.data, len(pairs) if npairs is None else npairs,
                                  None if edges is None else edges.ctypes.data, ne,
                                  None if hist is None else hist.ctypes.data, None)
    err = lambda: lib.bh_last_error()
    assert call(D=None) == E and call(nrows=0, start=(0, 0, 0)) == E and b'empty' in err()
    assert call(nrows=(1 << 32) + 1, start=(0, 4, (1 << 32) + 1)) == E
    assert call(stride=4) == E and b'stride' in err() and call(ncols=0) == E
    assert call(nsets=0) == E and b'sets' in err() and call(nsets=65536) == E
    assert call(start=None) == E
    assert call(start=(0, 6, 4, 10), nsets=3) == E and b'ascending' in err()
    assert call(start=(0, 4, 9)) == E and b'end at nrows' in err()
    assert call(start=(1, 4, 10)) == E
    assert call(pairs=[(0, 1)] * 17) == E and b'pairs' in err()
    assert call(npairs=0) == E and b'pairs' in err() and call(pairs=None, npairs=2) == E
    assert call(ne=1) == E and b'edges' in err() and call(ne=66) == E and b'edges' in err()
    assert call(edges=None) == E and call(hist=None) == E
    assert call(pairs=[(0, 5)]) == E and b'out of range' in err() and call(pairs=[(-1, 0)]) == E and b'out of range' in err()
    bad = edges.copy()
    bad[1, 3, 2] = bad[1, 3, 1]
    assert call(edges=bad) == E and b'ascending' in err()
    bad[1, 3, 2] = edges[1, 3, 2]
    bad[0, 0, 5] = np.nan
    assert call(edges=bad, pairs=[(0, 1)]) == E and b'ascending' in err()


def test_python_layer_refuses_bad_arguments():
    from bayhunter_amd import moho, scalars
    cols = scalars.Columns(np.zeros((10, 2)), ['f8', 'f8'])
    for start in ([0, 6, 4, 10], [0, 4, 9], [1, 10], [0]):
        with pytest.raises(ValueError, match='set_start'):
            scalars.summarize_sets(cols, start, device='cpu')
    with pytest.raises(ValueError, match='one weight per row'):
        scalars.summarize(cols, weights=np.ones(9, dtype=np.int32), device='cpu')
    with pytest.raises(ValueError, match='nbins <= 64'):
        moho.summarize_sets(np.zeros((10, 4)), [0, 10], moho=(20., 50.), nbins=65, device='cpu', tradeoff=True)


def test_pairs_kernel_uses_no_scratch_and_fits_the_lds(psim):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    r = kernel_resources('pairs.hip')
    mine = {k: v for k, v in r.items() if 'hist2d_sets_kernel' in k}
    assert len(mine) == 1, sorted(r)
    assert all(v['scratch'] == 0 for v in r.values()), r
    g = C.c_int(0)
    dyn = psim.ps_plan(32, 65, 16, C.byref(g))                    # 16 pairs of 32 distinct columns x 64 bins
    for k, v in mine.items():
        assert v['lds'] == psim.ps_static_lds(), (k, v)
        assert v['lds'] + dyn <= 64 * 1024, (k, v, dyn)
