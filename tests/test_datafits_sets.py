"""CPU tier of the segmented data-fit statistics (bh_datafits_sets_*, datafits.summarize_sets, StationPool.datafits):

* the new entry points refuse bad arguments before a device is touched (fake device pointers: nothing is launched);
* a hand-made table pins the ranks and the histogram edges every station gets from its own weight total and range;
* the chunk plan of the radix select (datafits_kernel.h, compiled with g++) never splits a set and covers every set once;
* summarize_sets takes the stations in runs of whole stations that fit max_rows, and no result depends on the runs;
* StationDatafits is assembled from the per-station dicts, checked against the numpy restatement (tests/datafits_ref.py)
  with a numpy stand-in for the device (the forward matrix and the sets handle);
* the kernels of datafits.hip use no scratch, and df_block stays within the registers df_kernel had before the segmented form.
"""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import datafits_ref as ref  # noqa: E402
from datafits_tolerances import STD_ATOL, STD_RTOL, check_mean, check_percentile  # noqa: E402

Q = (2.5, 16, 50, 84, 97.5)


# ---- the C ABI without a device -----------------------------------------------------------------------------

def test_datafits_sets_validates_arguments_without_gpu(lib):
    from bayhunter_amd import _lib
    start = np.array([0, 3, 3, 10], dtype=np.int64)
    h = C.c_void_p()

    def create(Y=1, nrows=10, stride=5, ncols=5, err=None, nerr=0, set_start=start, nsets=3, out=C.byref(h)):
        return lib.bh_datafits_sets_create(Y, nrows, stride, ncols, None, err, nerr,
                                           None if set_start is None else set_start.ctypes.data, nsets, None, out)
    for kw, words in ((dict(out=None), b'fits is NULL'), (dict(Y=None), b'no rows (empty selection)'),
                      (dict(nrows=0), b'no rows (empty selection)'), (dict(nrows=(1 << 32) + 1), b'2^32 rows'),
                      (dict(ncols=0), b'ncols < 1'), (dict(stride=4), b'stride < ncols'),
                      (dict(err=1, nerr=0), b'nerr < 1'), (dict(nsets=0), b'1 to 65535 sets'),
                      (dict(nsets=65536), b'1 to 65535 sets'), (dict(set_start=None), b'begin at 0 and end at nrows'),
                      (dict(set_start=np.array([1, 3, 3, 10], dtype=np.int64)), b'begin at 0'),
                      (dict(set_start=np.array([0, 3, 3, 9], dtype=np.int64)), b'end at nrows'),
                      (dict(set_start=np.array([0, 5, 3, 10], dtype=np.int64)), b'ascending')):
        assert create(**kw) == _lib.BH_ERR_ARG and words in lib.bh_last_error(), words
    assert not h.value
    status = np.zeros(3, dtype=np.int32)
    assert lib.bh_datafits_sets_scan(None, None, None, None, None, None, status.ctypes.data) == _lib.BH_ERR_ARG
    assert b'fits is NULL' in lib.bh_last_error()
    assert lib.bh_datafits_sets_set_chunk_bytes(None, 1 << 20) == _lib.BH_ERR_ARG
    lib.bh_datafits_sets_destroy(None)
    ranks, ost = np.zeros((3, 17), dtype=np.int64), np.zeros((3, 17, 5))
    edges, eset, hist = np.zeros((3, 1, 4)), np.zeros(5, dtype=np.int32), np.zeros((3, 5, 3), dtype=np.int64)

    def finish(ranks=ranks.ctypes.data, nranks=2, ost=ost.ctypes.data, edges=edges.ctypes.data, nedges=4, nesets=1,
               eset=eset.ctypes.data, hist=hist.ctypes.data):
        return lib.bh_datafits_sets_finish(None, ranks, nranks, ost, edges, nedges, nesets, eset, hist, None)
    for kw, words in ((dict(nranks=17), b'0 to 16 ranks'), (dict(nranks=-1), b'0 to 16 ranks'),
                      (dict(ost=None), b'ranks and order_stats'), (dict(ranks=None), b'ranks and order_stats'),
                      (dict(nedges=1), b'nedges >= 2'), (dict(nesets=0), b'nsets >= 1'), (dict(eset=None), b'eset'),
                      (dict(hist=None), b'hist'), (dict(), b'fits is NULL')):       # the last: all else in order
        assert finish(**kw) == _lib.BH_ERR_ARG and words in lib.bh_last_error(), words
    assert lib.bh_datafits_sets_status_text(0) == b''
    assert b'empty selection' in lib.bh_datafits_sets_status_text(1) and b'2^53' in lib.bh_datafits_sets_status_text(2)


def test_forward_batch_sets_validates_arguments_without_gpu(lib):
    from bayhunter_amd import _lib
    rf = (_lib.RfParams * 1)(_lib.RfParams(6.4, 1.0, 5.0, 5.0, -1.0, 512, 0, 201, 0))

    def call(B=4, nrf=1, nsets=3, table=1, set_id=1, out=1):
        return lib.bh_forward_batch_sets(B, 8, 8, 1, 1, 1, 1, 1, 0, None, None, 0, None, nrf, rf, None, 0.0, 1, out, 201, 1,
                                         None, 0, None, None, nsets, table, set_id)
    assert call(B=0) == _lib.BH_OK                                                   # nothing to do
    assert call(nsets=0) == _lib.BH_ERR_ARG and b'nsets < 1' in lib.bh_last_error()
    assert call(set_id=None) == _lib.BH_ERR_ARG and b'set_id is NULL' in lib.bh_last_error()
    assert call(nrf=0) == _lib.BH_ERR_ARG and b'without a receiver-function target' in lib.bh_last_error()
    assert call(out=None) == _lib.BH_ERR_ARG and b'NULL pointer' in lib.bh_last_error()     # bh_forward_batch's own
    assert call(B=0, table=None, nsets=-3, set_id=None) == _lib.BH_OK                # no table: bh_forward_batch


# ---- ranks and edges per station ----------------------------------------------------------------------------

def test_ranks_and_edges_per_station_hand_made():
    from bayhunter_amd.datafits import lerp, set_ranks, target_edges
    q = (25, 50, 75)
    rk, ranks = set_ranks(q, [1, 2, 10, 0, 101])
    assert np.array_equal(ranks, [[0, 0, 0, 0, 0, 0],            # W = 1: everything is rank 0
                                  [0, 1, 1, 1, 1, 1],            # W = 2: virtual indices .25 .5 .75 between 0 and 1
                                  [2, 3, 4, 5, 6, 7],            # W = 10: 2.25, 4.5, 6.75; the median's 4 and 5
                                  [0, 0, 0, 0, 0, 0],            # no weight: no ranks (the set is skipped)
                                  [25, 50, 75, 75, 75, 75]])     # W = 101: exact; filled up with the last rank
    assert ranks.dtype == np.int64 and rk[3] is None
    assert [r[4].tolist() for r in rk if r is not None] == [[0], [0, 1], [2, 3, 4, 5, 6, 7], [25, 50, 75]]
    for W, r in zip((1, 2, 10, 101), (rk[0], rk[1], rk[2], rk[4])):                 # numpy's percentile of 0..W-1
        virt, lo, hi, med, _ = r
        col = np.arange(W, dtype=np.float64)
        assert np.array_equal(lerp(col[lo], col[hi], virt - lo), np.percentile(col, q))
        assert (col[med[0]] + col[med[1]]) / 2 == np.median(col)
    with pytest.raises(ValueError, match='too many percentiles'):
        set_ranks(np.linspace(1, 99, 9), [1000])
    edges, eset = target_edges(np.array([1., 2., 5., 5., 5.]), np.array([3., 4., 5., 5., 5.]), [(0, 2), (2, 5)], 4)
    assert np.array_equal(edges, [[1, 1.75, 2.5, 3.25, 4], [4.5, 4.75, 5, 5.25, 5.5]])
    assert np.array_equal(eset, [0, 0, 1, 1, 1]) and eset.dtype == np.int32


# ---- launch geometry and the chunk plan ---------------------------------------------------------------------

@pytest.fixture(scope='module')
def dfsim():
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so = os.path.join(d, 'libdatafits_sets_sim.so')
    srcs = [os.path.join(d, 'datafits_sets_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h)
                                                         for h in ('datafits_kernel.h', 'posterior_kernel.h',
                                                                   'posterior_core.h', 'stats_core.h', 'bh_common.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so, srcs[0]], check=True)
    sim = C.CDLL(so)
    sim.dfs_blocks_of.argtypes = [C.c_longlong]
    sim.dfs_sets_per_chunk.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong]
    sim.dfs_chunks.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    sim.pos_blocks_of.argtypes = [C.c_longlong]
    sim.sets_slab_offsets.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return sim


def test_blocks_of_a_set_are_those_of_a_single_handle(dfsim):
    for rows, blocks in ((0, 0), (1, 1), (31, 1), (32, 1), (33, 2), (64, 2), (65, 3), (32 * 1024, 1024),
                         (32 * 1024 + 5, 1024), (1 << 32, 1024)):
        assert dfsim.dfs_blocks_of(rows) == blocks, rows


@pytest.mark.parametrize('posterior', [0, 1])
def test_slab_offsets_give_every_set_the_blocks_of_a_single_handle(dfsim, posterior):
    """The compact slab of the segmented reductions (SetStats::alloc_sets): set z owns goff[z] .. goff[z + 1], as many
    rows as the file's own blocks_of gives a handle over the set's rows -- row counts around both files' rows per block
    (32 and 256) and caps (1024 blocks) -- an empty set none, and goff[nsets] rows are the slab."""
    blocks_of = dfsim.pos_blocks_of if posterior else dfsim.dfs_blocks_of
    per_block = 256 if posterior else 32
    rows = np.array([0, 1, 31, 32, 33, 255, 256, 257, 0, 32 * 1024 + 5, 256 * 1024 + 1, 0], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    goff = np.full(rows.size + 1, -1, dtype=np.int64)
    gmax = dfsim.sets_slab_offsets(posterior, start.ctypes.data, rows.size, goff.ctypes.data)
    want = np.minimum(-(-rows // per_block), 1024)                     # ceil(rows / rows per block), capped
    assert [blocks_of(int(r)) for r in rows] == want.tolist()
    assert goff[0] == 0 and np.array_equal(np.diff(goff), want)
    assert np.all(np.diff(goff)[rows == 0] == 0)                       # an empty set owns no slab row
    assert goff[-1] == want.sum() and gmax == want.max() == 1024
    # sets that are all empty still launch one block column
    assert dfsim.sets_slab_offsets(posterior, np.zeros(4, dtype=np.int64).ctypes.data, 3, goff.ctypes.data) == 1
    assert goff[:4].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize('nsets,ncols,nranks,budget', [(7, 17, 12, 2 * 17 * 12 * 2048 + 1), (7, 17, 12, 1), (7, 17, 12, 0),
                                                        (1024, 222, 12, 0), (1, 1, 1, 0), (65535, 1, 16, 1 << 40),
                                                        (65535, 1, 4, 1 << 40), (100, 9, 5, 3 * 9 * 5 * 2048)])
def test_chunks_never_split_a_set_and_cover_every_set_once(dfsim, nsets, ncols, nranks, budget):
    first = np.zeros(nsets + 1, dtype=np.int32)
    n = dfsim.dfs_chunks(nsets, ncols, nranks, budget, first.ctypes.data)
    first = first[:n + 1]
    assert first[0] == 0 and first[-1] == nsets and np.all(np.diff(first) >= 1)     # whole sets, each once, in order
    size = np.diff(first)
    limit = budget if budget > 0 else 64 << 20
    table = size.astype(np.int64) * ncols * nranks * 2048
    assert np.all((table <= limit) | (size == 1))                                   # under the budget, or one set
    gz = -(-nranks // 4)
    assert np.all(size * gz <= 65535)                                               # the grid's z extent
    if budget > 0 and nsets > 1 and limit >= 2 * ncols * nranks * 2048:
        assert size.max() >= 2
    assert dfsim.dfs_sets_per_chunk(7, 17, 12, 3, 2 * 17 * 12 * 2048 + 1) == 2         # the GPU test's four chunks


# ---- runs of whole stations ---------------------------------------------------------------------------------

def test_station_runs_take_whole_stations():
    from bayhunter_amd.datafits import station_runs
    start = [0, 5, 5, 12, 20, 21]
    assert station_runs(start, 8) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert station_runs(start, 3) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]       # larger than max_rows: on its own
    assert station_runs(start, 12) == [(0, 3), (3, 5)]
    assert station_runs(start, 21) == station_runs(start, 10 ** 9) == [(0, 5)]
    assert station_runs([0, 0], 4) == [(0, 1)]
    with pytest.raises(ValueError):
        station_runs(start, 0)
    rs = np.random.RandomState(3)
    for _ in range(50):
        start = np.concatenate(([0], np.cumsum(rs.randint(0, 9, rs.randint(1, 12)))))
        cap = int(rs.randint(1, 20))
        runs = station_runs(start, cap)
        assert [a for a, _ in runs] + [runs[-1][1]] == [0] + [b for _, b in runs]    # contiguous, every set once
        assert runs[-1][1] == start.size - 1
        for a, b in runs:
            assert start[b] - start[a] <= cap or b == a + 1


# ---- a numpy stand-in for the device ------------------------------------------------------------------------

class _NumpyFits(object):
    """the sets handle in numpy (tests/datafits_ref.py)"""

    def __init__(self, Y, err, w, start):
        self.Y, self.start = Y, np.asarray(start)
        self.w = np.ones(Y.shape[0], dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
        assert (self.w >= 0).all()
        self.ok = ref.included(Y, err)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _rows(self, z):
        a, b = self.start[z], self.start[z + 1]
        use = self.ok[a:b] & (self.w[a:b] > 0)
        return self.Y[a:b][use], self.w[a:b][use]

    def scan(self):
        S, N = self.start.size - 1, self.Y.shape[1]
        out = dict(total=np.zeros(S, dtype=np.int64), excluded=np.zeros(S, dtype=np.int64), status=np.zeros(S, dtype=np.int32),
                   vmin=np.full((S, N), np.nan), vmax=np.full((S, N), np.nan), mean=np.full((S, N), np.nan))
        for z in range(S):
            a, b = self.start[z], self.start[z + 1]
            Y, w = self._rows(z)
            out['excluded'][z] = self.w[a:b][~self.ok[a:b]].sum()
            out['total'][z] = w.sum()
            out['status'][z] = 0 if w.sum() else 1
            if w.sum():
                out['vmin'][z], out['vmax'][z] = Y.min(axis=0), Y.max(axis=0)
                out['mean'][z] = (w[:, None] * Y).sum(axis=0) / w.sum()
        self.s = out
        return out

    def finish(self, ranks, edges, eset):
        S, N = self.start.size - 1, self.Y.shape[1]
        ost = np.full((S, ranks.shape[1], N), np.nan)
        hist = np.zeros((S, N, edges.shape[2] - 1), dtype=np.int64)
        std = np.full((S, N), np.nan)
        for z in range(S):
            if self.s['status'][z]:
                continue
            Y, w = self._rows(z)
            ost[z] = ref.order_stats(Y, w, ranks[z])
            hist[z] = [ref.histogram(Y[:, c], w, edges[z][eset[c]]) for c in range(N)]
            std[z] = np.sqrt((w[:, None] * (Y - self.s['mean'][z]) ** 2).sum(axis=0) / w.sum())
        return ost, hist, std

    def status_text(self, status):
        return "empty selection (no included row with a positive weight)"


class _NumpyBackend(object):
    """_DeviceSets in numpy: column c of the "modelled data" of a row is a fixed function of the row's model, its vp/vs
    and (with rf_p) its station's ray parameter, so a station's rows do not depend on the run they are modelled in."""
    segs, ncols = [(0, 4), (4, 9)], 9

    def __init__(self, rf_p=None, cap=10 ** 9):
        self.rf_p, self.cap, self.calls = rf_p, cap, []

    def max_rows(self):
        return self.cap

    def device(self):
        return contextlib.nullcontext()

    def forward(self, models, vpvs, set_id):
        m = np.asarray(models, dtype=np.float64)
        self.calls.append(m.shape[0])
        base = np.nansum(m, axis=1) * 0.01 + np.broadcast_to(np.asarray(vpvs, dtype=np.float64), (m.shape[0],))
        Y = np.sin(base[:, None] * (1 + np.arange(self.ncols))) + np.arange(self.ncols)
        if self.rf_p is not None:
            Y[:, 4:] += np.asarray(self.rf_p)[np.asarray(set_id), 0][:, None]
        Y[np.nansum(m, axis=1) > 290] = np.nan                     # a few rows whose modelled data are NaN
        err = (np.nanmax(m, axis=1) > 59.5).astype(np.int32)[:, None]     # ... and a few failed searches
        return Y, err

    def fits(self, Y, err, w, start):
        return _NumpyFits(Y, err, w, start)

    def gather(self, Y, idx):
        return Y[np.asarray(idx, dtype=np.int64)]


def _joint(rs, gap=False):
    """what _result reads of a JointTarget: two targets of 4 and 5 samples"""
    tg = []
    for ref_, n in (('rdispph', 4), ('prf', 5)):
        y = rs.normal(0, 1, n)
        if gap and ref_ == 'rdispph':
            y[2] = np.nan
        tg.append(types.SimpleNamespace(ref=ref_, obsdata=types.SimpleNamespace(x=np.arange(n, dtype=np.float64), y=y)))
    return types.SimpleNamespace(targets=tg, ntargets=2)


def _rows(rs, R, maxn=6):
    m = np.full((R, 2 * maxn), np.nan, dtype=np.float32)
    n = rs.randint(2, maxn + 1, R)
    for r in range(R):
        m[r, :n[r]] = rs.uniform(2, 5, n[r])
        m[r, n[r]:2 * n[r]] = np.sort(rs.uniform(0, 60, n[r]))
    return m


def _same(a, b, path=''):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], path + '/' + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (path, i))
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert np.array_equal(x, y, equal_nan=x.dtype.kind in 'fc'), path


def test_summarize_sets_does_not_depend_on_the_runs():
    from bayhunter_amd.datafits import _summarize_sets
    rs = np.random.RandomState(8)
    sizes = [40, 0, 25, 61, 1, 33]
    start = np.concatenate(([0], np.cumsum(sizes)))
    R = int(start[-1])
    models, vpvs = _rows(rs, R), rs.uniform(1.6, 1.9, R)
    w, mis = rs.randint(0, 7, R).astype(np.int32), rs.uniform(0, 1, R)
    w[start[4]] = 3
    stations = [_joint(rs) for _ in sizes]
    rf_p = np.linspace(4, 9, len(sizes))[:, None]
    out = []
    for cap in (10 ** 9, 70, 1):
        be = _NumpyBackend(rf_p, cap)
        got = _summarize_sets(stations, models, start, vpvs, w, mis, None, Q, 20, None, rf_p, None, backend=be)
        assert sorted(got.failed) == [1] and got[1] is None and 'empty selection' in got.failed[1]
        out.append((got, be.calls))
    assert out[0][1] == [R] and out[1][1] == [65, 62, 33] and out[2][1] == [40, 25, 61, 1, 33]
    forced = _summarize_sets(stations, models, start, vpvs, w, mis, None, Q, 20, None, rf_p, 70, backend=_NumpyBackend(rf_p))
    for other in (out[1][0], out[2][0], forced):
        _same(list(other), list(out[0][0]))
    # every station against the restatement on its own rows
    be = _NumpyBackend(rf_p)
    for z in (0, 2, 3, 4, 5):
        a, b = start[z], start[z + 1]
        Y, err = be.forward(models[a:b], vpvs[a:b], np.full(b - a, z))
        want = ref.summarize(Y, w[a:b], Q, segs=be.segs, nbins=20, err=err)
        res = out[0][0][z]
        assert res['nmodels'] == want['nmodels'] and res['nexcluded'] == want['nexcluded']
        cand = np.nonzero(w[a:b] > 0)[0]
        best = Y[cand[np.argmin(mis[a:b][cand])]]
        for t, (c0, c1), e in zip(res['targets'], be.segs, want['edges']):
            for k in ('min', 'max', 'median'):
                assert np.array_equal(t[k], want[k][c0:c1]), (z, k)
            check_percentile(t['quantiles'], want['quantiles'][:, c0:c1], want['lower'][:, c0:c1], want['upper'][:, c0:c1])
            np.testing.assert_allclose(t['std'], want['std'][c0:c1], rtol=STD_RTOL, atol=STD_ATOL)
            assert np.array_equal(t['density'][0], want['hist'][c0:c1]) and np.array_equal(t['density'][1], e)
            assert np.array_equal(t['best'], best[c0:c1], equal_nan=True)
            assert np.array_equal(t['residual'], t['yobs'] - best[c0:c1], equal_nan=True)
        ok = ref.included(Y, err) & (w[a:b] > 0)
        check_mean(np.concatenate([t['mean'] for t in res['targets']]), Y[ok], w[a:b][ok])


def _fake_station_pool(rs, S, c, nrows, per_station=()):
    """what stations_datafits reads of a StationPool: chains of `nrows` saved rows, the main phase from row 2 on"""
    nch = S * c
    it = np.tile(np.arange(-2, nrows - 2, dtype=np.float64) * 3, (nch, 1))
    pool = types.SimpleNamespace(
        nchains=nch, first=0, iter=it, iter_main=3 * (nrows - 2) + 2, priors={}, initparams=dict(maxmodels=50),
        models=np.stack([_rows(rs, nrows) for _ in range(nch)]), vpvs=rs.uniform(1.6, 1.9, (nch, nrows)).astype(np.float32),
        misfits=rs.uniform(0, 1, (nch, nrows, 3)).astype(np.float32), likes=rs.uniform(1, 2, (nch, nrows)).astype(np.float32),
        counters=lambda: (np.full(nch, nrows),))
    names = ['S%d' % s for s in range(S)]
    return types.SimpleNamespace(pool=pool, chains_per_station=c, names=names, per_station=per_station,
                                 stations=[_joint(rs, gap=(s == 1)) for s in range(S)])


def test_station_datafits_assembly_with_a_numpy_matrix():
    from bayhunter_amd.datafits import best_rows, stations_datafits
    from bayhunter_amd.selection import station_rows
    rs = np.random.RandomState(12)
    S, c, nrows = 4, 3, 9
    sp = _fake_station_pool(rs, S, c, nrows)
    sp.pool.iter[2 * c:3 * c] = -1                                  # station 2: no main-phase row
    with pytest.raises(ValueError, match="station 'S2'.*empty selection"):
        stations_datafits(sp, exclude_outliers=False, backend=_NumpyBackend(), nbins=10)
    res = stations_datafits(sp, exclude_outliers=False, backend=_NumpyBackend(), nbins=10, strict=False)
    runs = stations_datafits(sp, exclude_outliers=False, backend=_NumpyBackend(), nbins=10, strict=False, max_rows=25)
    assert res.names == sp.names and list(res.stations) == ['S0', 'S1', 'S3'] and list(res.failed) == ['S2']
    assert 'empty selection' in res.failed['S2'] and res.refs == ['rdispph', 'prf']
    _same(runs.stations, res.stations)
    ci, ri, w, start, _ = station_rows(sp.pool, c, 'weighted', 0.05, False)
    assert list(np.diff(start)) == [21, 21, 0, 21] and np.all(w[ci // c != 2] > 0)
    be = _NumpyBackend()
    for z, name in enumerate(sp.names):
        if z == 2:
            for k in res.FIELDS:
                assert all(np.isnan(a[z]).all() for a in getattr(res, k))
            assert all(np.isnan(a[z]).all() for a in res.quantiles) and res.nmodels[z] == 0 and res.nexcluded[z] == 0
            continue
        a, b = start[z], start[z + 1]
        r = res.stations[name]
        Y, err = be.forward(sp.pool.models[ci[a:b], ri[a:b]], sp.pool.vpvs[ci[a:b], ri[a:b]].astype(np.float64), None)
        want = ref.summarize(Y, w[a:b], Q, segs=be.segs, nbins=10, err=err)
        assert r['nmodels'] == want['nmodels'] == res.nmodels[z] and r['nexcluded'] == want['nexcluded'] == res.nexcluded[z]
        assert set(r) == {'targets', 'q', 'nmodels', 'nexcluded', 'bestfits', 'chains'}
        assert np.array_equal(r['chains'], np.arange(c)) and np.array_equal(r['bestfits']['chains'], np.arange(c))
        mis = sp.pool.misfits[ci[a:b], ri[a:b], -1].astype(np.float64)
        pick = best_rows(ci[a:b], w[a:b], mis)
        assert np.array_equal(r['bestfits']['rows'], ri[a:b][pick])
        for t, ((c0, c1), d) in enumerate(zip(be.segs, r['targets'])):
            assert np.array_equal(r['bestfits']['data'][t], Y[pick][:, c0:c1], equal_nan=True)
            assert np.array_equal(d['median'], want['median'][c0:c1]) and np.array_equal(d['min'], want['min'][c0:c1])
            assert np.array_equal(d['density'][0], want['hist'][c0:c1])
            assert np.array_equal(d['best'], Y[np.argmin(mis)][c0:c1], equal_nan=True)
            for k in res.FIELDS:                                    # the stacked arrays are the per-station fields
                assert np.array_equal(getattr(res, k)[t][z], d[k], equal_nan=True), (name, k)
            assert np.array_equal(res.quantiles[t][z], d['quantiles'])
            assert getattr(res, 'mean')[t].shape == (S, c1 - c0) and res.quantiles[t].shape == (S, len(Q), c1 - c0)
        if z == 1:                                                  # the gap: observed value and residual NaN there only
            d = r['targets'][0]
            assert np.isnan(d['yobs'][2]) and np.isnan(d['residual'][2]) and np.isfinite(np.delete(d['residual'], 2)).all()
            assert np.isfinite(d['mean']).all() and np.isnan(res.residual[0][1, 2])


# ---- the kernels' budget ------------------------------------------------------------------------------------

# next_free_vgpr of datafits.hip's kernels read from a build of commit 3323cf2 (the parent of the segmented form)
PARENT_VGPR = {'df_kernelILi1E': 28, 'df_kernelILi2E': 26, 'df_kernelILi3E': 26, 'df_mask_kernel': 28}


def test_sets_kernels_use_no_scratch_and_df_kernel_did_not_grow():
    """df_kernel itself is gone (a bh_datafits handle is the single set of df_sets_kernel); its body, df_block, is held
    to what df_kernel had there: the mode's registers rounded up to the allocation granule of 8."""
    from kernel_resources import kernel_resources
    sets = kernel_resources('datafits.hip')
    mine = {k: v for k, v in sets.items() if 'df_sets_' in k or 'stats_sets_reduce_kernel' in k}
    assert len(mine) == 5, sorted(sets)                              # mask, the shared reduce and the three modes
    assert len([k for k in mine if 'df_sets_' in k]) == 4, sorted(mine)
    for name, row in mine.items():
        assert row['scratch'] == 0, (name, row)
    for mode in ('ILi1E', 'ILi2E', 'ILi3E'):
        rows = [v for k, v in mine.items() if 'df_sets_kernel' + mode in k]
        assert len(rows) == 1, (mode, sorted(mine))
        assert rows[0]['vgpr'] <= -(-PARENT_VGPR['df_kernel' + mode] // 8) * 8, (mode, rows[0])
