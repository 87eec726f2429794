"""GPU tier of the segmented velocity-depth posterior (bh_posterior_sets_*, posterior.summarize_sets,
StationPool.posterior).

The oracle is the single-set path: for every set, every field of summarize_sets equals what posterior.summarize
returns for that set's rows alone, bit for bit -- mean and standard deviation included.  There is no tolerance in
this file, no set and no field is skipped, and every set outside the deliberately failed ones has a single-set
result (summarize raises otherwise)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
from test_posterior import random_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEP = np.linspace(0, 60, 61)                  # 61 depths: no multiple of the kernel's tile of 8
FIELDS = {'singlemodels', 'hist2d', 'interfaces', 'nlayers', 'nmodels'}
SINGLE = {'mean', 'median', 'minmax', 'stdminmax', 'mode', 'minmisfit'}
SIZES = (1, 255, 256, 257, 513, 262145)       # the last one: more than 1 024 blocks of 256 rows, capped for it alone


def assert_equal_trees(a, b, path=''):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            assert_equal_trees(a[k], b[k], '%s/%s' % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            assert_equal_trees(x, y, '%s[%d]' % (path, i))
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype, path
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind in 'fc' else np.array_equal(x, y), path


def singles(rows, start, w=None, mis=None, dep=DEP, only=None):
    """summarize() of every set's rows alone (of the sets `only`)."""
    from bayhunter_amd.posterior import summarize
    out = {}
    for z in (range(len(start) - 1) if only is None else only):
        sl = slice(start[z], start[z + 1])
        out[z] = summarize(rows[sl], None if w is None else w[sl], dep_int=dep, misfits=None if mis is None else mis[sl])
    return out


def assert_sets_equal_singles(res, want, nsets, with_misfit=True):
    assert len(res) == nsets and not res.failed
    compared = 0
    for z in range(nsets):
        assert set(res[z]) == FIELDS and set(res[z]['singlemodels']) == (SINGLE if with_misfit else SINGLE - {'minmisfit'})
        assert_equal_trees(res[z], want[z], 'set %d' % z)
        compared += 1
    assert compared == nsets == len(want)


def scale_vs(rows, lo, hi):
    """The Vs half of every row mapped from random_rows' 1..5 km/s to lo..hi."""
    rows = rows.copy()
    n = (~np.isnan(rows)).sum(axis=1) // 2
    m = np.arange(rows.shape[1])[None, :] < n[:, None]
    rows[m] = lo + (rows[m] - 1.0) * ((hi - lo) / 4.0)
    return rows


_boundary = {}


def boundary_case(dtype):
    """Sets of SIZES rows of random_rows (width 16): weights 0..300 with zeros, all-NaN rows, misfits with a NaN and
    with ties across block boundaries -> the inputs, summarize() per set, and summarize_sets()."""
    if dtype in _boundary:
        return _boundary[dtype]
    from bayhunter_amd.posterior import summarize_sets
    rs = np.random.RandomState(77)
    start = np.concatenate(([0], np.cumsum(SIZES)))
    R = int(start[-1])
    base = random_rows(rs, 20000, width=16)
    rows = base[rs.randint(0, base.shape[0], R)]
    w = rs.randint(0, 301, R).astype(np.int32)
    w[rs.rand(R) < 0.05] = 0
    rows[rs.rand(R) < 0.01] = np.nan
    rows[0] = np.nan                                                  # the set of one row: three layers, weight 7
    rows[0, :3], rows[0, 3:6] = (2.0, 3.0, 4.0), (5.0, 20.0, 40.0)
    w[0] = 7
    mis = np.round(rs.uniform(1, 2, R), 2)                            # ties everywhere
    s513 = int(start[4])
    mis[s513:s513 + 513] += 1.0
    for r in (255, 256, 512):                                         # the least value on both sides of a block boundary
        mis[s513 + r], w[s513 + r] = 0.5, 3
        rows[s513 + r] = base[r]
    s257 = int(start[3])
    mis[s257 + 256], w[s257 + 256], rows[s257 + 256] = np.nan, 2, base[7]     # np.argmin: the first NaN wins
    big = int(start[5])
    for r in (5, 255, 256, 70000, 262144):                            # ties across blocks of the capped set
        mis[big + r], w[big + r] = 0.25, 1
        rows[big + r] = base[r % 20000]
    rows = rows.astype(dtype)
    want = singles(rows, start, w, mis)
    got = summarize_sets(rows, start, w, dep_int=DEP, misfits=mis)
    _boundary[dtype] = dict(rows=rows, w=w, mis=mis, start=start, want=want, got=got)
    return _boundary[dtype]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_every_set_equals_summarize_of_its_rows(lib, dtype):
    import torch
    from bayhunter_amd.posterior import Grid, Sets
    k = boundary_case(dtype)
    assert_sets_equal_singles(k['got'], k['want'], len(SIZES))
    # the argmin itself: the single-set argmin plus the set's first row
    dev = torch.device('cuda')
    rows, w, mis = (torch.from_numpy(k[n]).to(dev) for n in ('rows', 'w', 'mis'))
    st = torch.cuda.current_stream().cuda_stream
    with Sets(rows, w, mis, k['start'], DEP, None, st) as sets:
        s = sets.scan()
    assert not s['status'].any()
    for z in range(len(SIZES)):
        a, b = int(k['start'][z]), int(k['start'][z + 1])
        with Grid(rows[a:b], w[a:b], mis[a:b], DEP, None, st) as one:
            s1 = one.scan()
        assert s['argmin'][z] == s1['argmin'] + a and s['total'][z] == s1['total']
    s513, s257, big = (int(k['start'][i]) for i in (4, 3, 5))
    assert s['argmin'][4] == s513 + 255 and s['argmin'][3] == s257 + 256 and s['argmin'][5] == big + 5


def test_chunks_change_no_bit_and_two_calls_are_identical(lib):
    from bayhunter_amd.posterior import summarize_sets
    k = boundary_case(np.float32)
    budget = 500000
    assert budget // (DEP.size * 2 * 256 * 8) == 2        # 6 sets: 3 chunks on the depth grid, 6 on the half-step grid
    a = summarize_sets(k['rows'], k['start'], k['w'], dep_int=DEP, misfits=k['mis'], chunk_bytes=budget)
    b = summarize_sets(k['rows'], k['start'], k['w'], dep_int=DEP, misfits=k['mis'], chunk_bytes=budget)
    assert len(a) == len(b) == len(SIZES)
    for z in range(len(SIZES)):
        assert_equal_trees(a[z], k['got'][z], 'chunked set %d' % z)
        assert_equal_trees(b[z], a[z], 'second call, set %d' % z)
    assert np.array_equal(a.std, k['got'].std)


@pytest.fixture(scope='module')
def edge_case():
    """Ordinary sets around one with Vs in 3.0..3.1 km/s (four mode bins) and one with Vs up to 30 km/s (more than
    1 024 Vs bins: the histogram tile does not fit the LDS, global atomics)."""
    rs = np.random.RandomState(78)
    sizes = (300, 200, 777, 400, 300)
    start = np.concatenate(([0], np.cumsum(sizes)))
    rows = random_rows(rs, int(start[-1]), width=16)
    rows[start[1]:start[2]] = scale_vs(rows[start[1]:start[2]], 3.0, 3.1)
    rows[start[3]:start[4]] = scale_vs(rows[start[3]:start[4]], 1.0, 30.0)
    w = rs.randint(0, 301, int(start[-1])).astype(np.int32)
    return rows, w, start


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_sets_with_their_own_vs_edges_and_both_histogram_paths(lib, edge_case, dtype):
    from bayhunter_amd.posterior import summarize_sets
    rows, w, start = edge_case
    rows = rows.astype(dtype)
    got = summarize_sets(rows, start, w, dep_int=DEP)
    want = singles(rows, start, w)
    assert_sets_equal_singles(got, want, 5, with_misfit=False)
    nbins = [r['hist2d'][0].shape[0] for r in got]
    assert nbins[1] < 12 and nbins[3] > 1024 and all(100 < n < 300 for n in (nbins[0], nbins[2], nbins[4]))
    assert got[1]['singlemodels']['mode'][0].size == 60 and len(set(nbins)) >= 3
    # an irregular depth grid
    dep = np.concatenate((np.arange(0, 10, 0.5), np.arange(10, 30, 2.5), [30., 31., 45., 60.]))
    got = summarize_sets(rows, start, w, dep_int=dep)
    assert_sets_equal_singles(got, singles(rows, start, w, dep=dep), 5, with_misfit=False)


def test_depth_tiles_wider_than_the_lds_histogram(lib, edge_case):
    """Depth bins 2 * d: a tile of 8 depths spans 15 bins, more than the LDS histogram's 8 rows, so every set takes
    the global-atomics path.  (summarize's own grids put two half-step depths into each bin and never get there,
    so the handles are driven directly.)"""
    import torch
    from bayhunter_amd.posterior import Grid, Sets, mode_edges
    rows, w, start = edge_case
    dev = torch.device('cuda')
    trows, tw = torch.from_numpy(rows.astype(np.float32)).to(dev), torch.from_numpy(w).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    dbin = (2 * np.arange(DEP.size)).astype(np.int32)
    dbin[5] = -1
    with Sets(trows, tw, None, start, DEP, None, st) as sets:
        s = sets.scan()
        edges = [mode_edges(s['vmin'][z], s['vmax'][z]) for z in range(5)]
        hists, std, med = sets.finish(edges, dbin, 2 * DEP.size, True)
    for z in range(5):
        a, b = int(start[z]), int(start[z + 1])
        with Grid(trows[a:b], tw[a:b], None, DEP, None, st) as one:
            s1 = one.scan()
            e1 = mode_edges(s1['vmin'], s1['vmax'])
            h1, std1, med1 = one.finish(e1, dbin, 2 * DEP.size, True)
        assert np.array_equal(e1, edges[z]) and np.array_equal(h1, hists[z]) and h1.sum() > 0
        assert np.array_equal(std1, std[z]) and np.array_equal(med1, med[z]) and np.array_equal(s1['mean'], s['mean'][z])


def test_failed_sets_between_live_ones(lib):
    from bayhunter_amd import _lib
    from bayhunter_amd.posterior import summarize, summarize_sets
    rs = np.random.RandomState(79)
    sizes = (300, 0, 257, 100, 50, 513)                   # live, empty, live, all weights 0, all Vs equal, live
    start = np.concatenate(([0], np.cumsum(sizes)))
    rows = random_rows(rs, int(start[-1]), width=16)
    w = rs.randint(1, 301, int(start[-1])).astype(np.int32)
    mis = rs.uniform(1, 2, int(start[-1]))
    w[start[3]:start[4]] = 0
    rows[start[4]:start[5]] = scale_vs(rows[start[4]:start[5]], 3.0, 3.02)
    rows = rows.astype(np.float32)
    got = summarize_sets(rows, start, w, dep_int=DEP, misfits=mis, strict=False)
    assert sorted(got.failed) == [1, 3, 4] and [r is None for r in got] == [False, True, False, True, True, False]
    assert 'empty selection' in got.failed[1] and 'empty selection' in got.failed[3] and '0.025' in got.failed[4]
    live = (0, 2, 5)
    want = singles(rows, start, w, mis, only=live)
    for z in live:
        assert set(got[z]) == FIELDS
        assert_equal_trees(got[z], want[z], 'set %d' % z)
    assert len(want) == 3
    # the single-set path fails the same sets
    for z in (3, 4):
        sl = slice(start[z], start[z + 1])
        with pytest.raises((ValueError, _lib.BayHunterAmdError)):
            summarize(rows[sl], w[sl], dep_int=DEP)
    sec = got.section()
    for z in range(6):
        for key in ('mean', 'median', 'std', 'vmin', 'vmax', 'mode'):
            assert np.isnan(sec[key][z]).all() if z in got.failed else np.isfinite(sec[key][z]).all(), (z, key)
    with pytest.raises(ValueError, match='set 1: empty selection'):
        summarize_sets(rows, start, w, dep_int=DEP, misfits=mis)
    w[start[5] + 300] = -1                                # a negative weight fails the whole call
    with pytest.raises(_lib.BayHunterAmdError, match='negative weight'):
        summarize_sets(rows, start, w, dep_int=DEP, misfits=mis, strict=False)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_compact_slab_with_empty_sets_between_multi_block_ones(lib, dtype):
    """Sets of 0, 1, 257, 0, 513 and 256 rows (G = 0, 1, 2, 0, 3, 1 slab rows, one after the other) in chunks of two
    sets on the depth grid: a chunk boundary between sets of different G, an empty set opening a chunk, an empty set
    between multi-block ones inside the slab.  The live sets equal summarize() of their rows, the empty ones fail with
    the scan's words, and the 513-row set's argmin -- planted in its second block -- comes back as that row."""
    import torch
    from bayhunter_amd.posterior import Sets, summarize_sets
    rs = np.random.RandomState(80)
    sizes = (0, 1, 257, 0, 513, 256)
    start = np.concatenate(([0], np.cumsum(sizes)))
    R = int(start[-1])
    rows = random_rows(rs, R, width=16)
    rows[0] = np.nan                                                  # the set of one row: three layers
    rows[0, :3], rows[0, 3:6] = (2.0, 3.0, 4.0), (5.0, 20.0, 40.0)
    rows = rows.astype(dtype)
    w = rs.randint(1, 301, R).astype(np.int32)
    mis = np.round(rs.uniform(1, 2, R), 2)
    planted = int(start[4]) + 256
    mis[planted] = 0.5
    budget = 500000
    assert budget // (DEP.size * 2 * 256 * 8) == 2
    got = summarize_sets(rows, start, w, dep_int=DEP, misfits=mis, strict=False, chunk_bytes=budget)
    assert len(got) == 6 and sorted(got.failed) == [0, 3] and got[0] is None and got[3] is None
    for z in (0, 3):
        assert got.failed[z] == 'empty selection (no included row with a positive weight)'
    live = (1, 2, 4, 5)
    want = singles(rows, start, w, mis, only=live)
    assert len(want) == 4
    for z in live:
        assert set(got[z]) == FIELDS and set(got[z]['singlemodels']) == SINGLE
        assert_equal_trees(got[z], want[z], 'set %d' % z)
    dev = torch.device('cuda')
    with Sets(torch.from_numpy(rows).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(mis).to(dev), start, DEP,
              None, torch.cuda.current_stream().cuda_stream, chunk_bytes=budget) as sets:
        s = sets.scan()
    assert s['status'].tolist() == [1, 0, 0, 1, 0, 0] and s['argmin'][4] == planted
    assert s['argmin'][0] == -1 and s['argmin'][3] == -1 and s['argmin'][1] == 0
    assert np.array_equal(s['total'], [w[start[z]:start[z + 1]].sum() for z in range(6)])


def test_station_pool_posterior_equals_every_station_views(lib):
    from bayhunter_amd.posterior import summarize_sets
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=150, iter_main=100)
    stations = make_stations(os.path.join(GOLDEN, 'tutorial_observed'), 3, refs=case.get('refs', ('rdispph', 'prf')), yerr=True)
    names = ['AAA', 'BBB', 'CCC']
    with StationPool(dict(zip(names, stations)), ip, case['priors'], chains_per_station=4, random_seeds=[21, 22, 23],
                     nmodels=251) as pool:
        pool.run()
    for kw in (dict(selection='weighted'), dict(selection='saved'), dict(selection='weighted', exclude_outliers=False)):
        res = pool.posterior(dev=0.5, **kw)
        assert not res.failed and list(res.stations) == names and res.names == names
        for s, name in enumerate(names):
            want = pool.station(name).posterior(dev=0.5, **kw)
            assert_equal_trees(res.stations[name], want, name)
            sm = want['singlemodels']
            assert np.array_equal(res.mean[s], sm['mean'][0]) and np.array_equal(res.median[s], sm['median'][0])
            assert np.array_equal(res.vmin[s], sm['minmax'][0][0]) and np.array_equal(res.vmax[s], sm['minmax'][0][1])
            assert np.array_equal(res.mode[s], sm['mode'][0]) and np.array_equal(res.dep, sm['mean'][1])
            assert np.array_equal(sm['mean'][0] + res.std[s], sm['stdminmax'][0][1])
        assert res.mean.shape == (3, res.dep.size) and res.mode.shape == (3, res.dep.size - 1)
    # a station whose rows are all NaN: a NaN row of the section, its neighbours untouched
    ci, ri = np.nonzero(pool.pool.iter >= 0)
    rows = pool.pool.models[ci, ri]
    st = np.searchsorted(ci // 4, np.arange(4))
    rows[st[1]:st[2]] = np.nan
    sets = summarize_sets(rows, st, dep_int=res.dep, strict=False)
    assert list(sets.failed) == [1] and sets[1] is None and sets[0] is not None and sets[2] is not None
    sec = sets.section()
    assert np.isnan(sec['mean'][1]).all() and np.isnan(sec['mode'][1]).all()
    assert np.array_equal(sec['mean'][0], sets[0]['singlemodels']['mean'][0]) and np.isfinite(sec['mean'][[0, 2]]).all()
