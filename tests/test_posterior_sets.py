"""CPU tier of the segmented velocity-depth posterior (bh_posterior_sets_*, posterior.summarize_sets,
StationPool.posterior):

* the radix select with one list of ranks per column (stats_core.h), compiled with g++ and fed numpy's digit
  histograms, finds the order statistics numpy's sort finds in columns of very different weight totals;
* the pool-wide selection and outlier step (selection.station_rows) gives every station the rows pool_rows gives
  its view;
* the C ABI refuses bad arguments before a device is touched (the kernels' budget: test_posterior.py).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))

TOTALS = (1, 2, 3, 255, 256, 1000, 2 ** 40 + 1)


@pytest.fixture(scope='module')
def pssim():
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so = os.path.join(d, 'libposterior_sets_sim.so')
    srcs = [os.path.join(d, 'posterior_sets_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h)
                                                          for h in ('stats_core.h', 'bh_common.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so, srcs[0]],
                       check=True)
    lib = C.CDLL(so)
    lib.pss_sel_new.restype = C.c_void_p
    return lib


def columns_with_totals(rs, dtype, totals=TOTALS):
    """Y [R, N] and weights W [R, N] (uint64; column c sums to totals[c], zeros among them), values with ties."""
    R, N = 40, len(totals)
    Y = np.round(rs.normal(0, 3, (R, N)), 1).astype(dtype)
    W = np.zeros((R, N), dtype=np.uint64)
    for c, tot in enumerate(totals):
        k = min(tot, R - 3)                               # rows of positive weight
        rows = rs.permutation(R)[:k]
        cuts = np.sort(rs.choice(np.arange(1, tot), k - 1, replace=False)) if tot < 10 ** 6 else \
            np.sort(rs.randint(1, tot, k - 1, dtype=np.int64))
        parts = np.diff(np.r_[0, cuts, tot]).astype(np.uint64)
        parts = parts[parts > 0] if tot >= 10 ** 6 else parts
        W[rows[:parts.size], c] = parts
        assert int(W[:, c].sum()) == tot
    return Y, W


def select(pssim, Y, W, ranks, per_column):
    """The keys' values at `ranks` ([nranks] shared, or [nranks, N] per column) of every weighted column of Y."""
    R, N = Y.shape
    bits = 8 * Y.dtype.itemsize
    K = np.zeros(Y.size, dtype=np.uint64 if bits == 64 else np.uint32)
    (pssim.pss_keys64 if bits == 64 else pssim.pss_keys32)(C.c_void_p(np.ascontiguousarray(Y).ctypes.data),
                                                          C.c_long(Y.size), C.c_void_p(K.ctypes.data))
    K = K.reshape(R, N).astype(np.uint64)
    ranks = np.ascontiguousarray(ranks, dtype=np.uint64)
    n = ranks.shape[0]
    sel = C.c_void_p(pssim.pss_sel_new(C.c_int(N), C.c_int(n), C.c_int(bits), C.c_void_p(ranks.ctypes.data),
                                       C.c_int(int(per_column))))
    gbase, ngroups, gpfx = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros(n * N, dtype=np.uint64)
    slots = C.c_int(0)
    passes = 0
    try:
        while True:
            shift = pssim.pss_sel_plan(sel, C.c_void_p(gbase.ctypes.data), C.c_void_p(ngroups.ctypes.data),
                                       C.c_void_p(gpfx.ctypes.data), C.byref(slots))
            if shift < 0:
                break
            passes += 1
            digits = np.zeros((slots.value, 256), dtype=np.uint64)
            for c in range(N):
                hi = np.zeros(R, dtype=np.uint64) if shift + 8 >= bits else K[:, c] >> np.uint64(shift + 8)
                dig = ((K[:, c] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
                for t in range(ngroups[c]):
                    m = hi == gpfx[gbase[c] + t]
                    np.add.at(digits[gbase[c] + t], dig[m], W[m, c])
            pssim.pss_sel_advance(sel, C.c_void_p(digits.ctypes.data))
        keys = np.zeros((n, N), dtype=np.uint64)
        pssim.pss_sel_keys(sel, C.c_void_p(keys.ctypes.data))
    finally:
        pssim.pss_sel_free(sel)
    assert passes == bits // 8
    out = np.zeros((n, N), dtype=Y.dtype)
    for i in range(n):
        for c in range(N):
            at = np.nonzero((K[:, c] == keys[i, c]) & (W[:, c] > 0))[0]
            assert at.size, 'rank %d of column %d: the key found is no key of the column' % (i, c)
            out[i, c] = Y[at[0], c]
    return out


def sorted_order_stat(y, w, rank):
    o = np.argsort(y, kind='stable')
    cum = np.cumsum(w[o].astype(object))                  # Python integers: totals above 2^40 without rounding
    return y[o[int(np.searchsorted(np.array([int(v) for v in cum], dtype=np.uint64), np.uint64(rank), side='right'))]]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_select_with_ranks_per_column_equals_numpy_sort(pssim, dtype):
    rs = np.random.RandomState(40)
    Y, W = columns_with_totals(rs, dtype)
    tot = np.array(TOTALS, dtype=np.uint64)
    ranks = np.stack(((tot - np.uint64(1)) // np.uint64(2), tot // np.uint64(2)))     # each column's two middle ranks
    got = select(pssim, Y, W, ranks, True)
    for c in range(len(TOTALS)):
        for i in range(2):
            assert got[i, c] == sorted_order_stat(Y[:, c], W[:, c], int(ranks[i, c])), (i, c)
    for c in range(3):                                    # totals 1, 2, 3 by hand: the expanded column is that short
        exp = np.sort(np.repeat(Y[:, c], W[:, c].astype(np.int64)))
        assert got[0, c] == exp[(TOTALS[c] - 1) // 2] and got[1, c] == exp[TOTALS[c] // 2]
    # first and last rank of every column
    ends = np.stack((np.zeros_like(tot), tot - np.uint64(1)))
    got = select(pssim, Y, W, ends, True)
    for c in range(len(TOTALS)):
        live = W[:, c] > 0
        assert got[0, c] == Y[live, c].min() and got[1, c] == Y[live, c].max()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_shared_rank_constructor_gives_what_it_gave(pssim, dtype):
    rs = np.random.RandomState(41)
    Y, W = columns_with_totals(rs, dtype, totals=(1000,) * 4)
    shared = np.array([0, 499, 500, 999], dtype=np.uint64)
    got = select(pssim, Y, W, shared, False)
    for c in range(4):
        for i, r in enumerate(shared):
            assert got[i, c] == sorted_order_stat(Y[:, c], W[:, c], int(r))
    assert np.array_equal(got, select(pssim, Y, W, np.repeat(shared[:, None], 4, axis=1), True))


@pytest.fixture(scope='module')
def station_pool(oracle):
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES, oracle_evaluator
    from station_scenario import make_stations, station_evaluator
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=90, iter_main=50)
    stations = make_stations(os.path.join(GOLDEN, 'tutorial_observed'), 3, oracle=oracle, yerr=True)
    ev = station_evaluator([oracle_evaluator(j) for j in stations])
    pool = StationPool(stations, ip, case['priors'], chains_per_station=4, random_seeds=[7, 8, 9], evaluator=ev,
                       nmodels=141).run()
    pool.pool.initparams['maxmodels'] = 13                # thinning > 1 in the 'saved' selection
    return pool


@pytest.mark.parametrize('selection', ['weighted', 'saved'])
@pytest.mark.parametrize('dev,exclude', [(0.05, True), (0.0005, True), (0.05, False)])
def test_station_rows_are_pool_rows_of_every_view(station_pool, selection, dev, exclude):
    from bayhunter_amd.selection import pool_outliers, pool_rows, station_rows
    pool, c = station_pool, station_pool.chains_per_station
    ci, ri, w, start, failed = station_rows(pool.pool, c, selection, dev, exclude)
    assert not failed and start.size == 4 and start[0] == 0 and start[-1] == ci.size
    dropped = 0
    for s in range(3):
        view = pool.station(s)
        wci, wri, ww = pool_rows(view, selection, dev, exclude)
        sl = slice(start[s], start[s + 1])
        assert np.array_equal(ci[sl] - s * c, wci) and np.array_equal(ri[sl], wri) and np.array_equal(w[sl], ww)
        assert w.dtype == ww.dtype
        dropped += pool_outliers(view, dev).size
    assert exclude is False or dev > 0.001 or dropped > 0  # the tight bound does leave chains out


def test_station_rows_fail_the_stations_pool_rows_refuses(station_pool):
    """A weight above int32 (here: every chain's last row, with a main phase declared 2^40 iterations long) is
    pool_rows' ValueError for the station's view and an entry of `failed` for that station, not an error of the call."""
    from bayhunter_amd.selection import pool_rows, station_rows
    inner = station_pool.pool
    keep = inner.iter_main
    inner.iter_main = 2 ** 40
    try:
        ci, ri, w, start, failed = station_rows(inner, 4, 'weighted', 0.05, False)
        assert sorted(failed) == [0, 1, 2] and all('2^31' in m for m in failed.values())
        assert ci.size == 0 and np.array_equal(start, [0, 0, 0, 0])
        with pytest.raises(ValueError, match='2\\^31'):
            pool_rows(station_pool.station(1), 'weighted', 0.05, False)
    finally:
        inner.iter_main = keep


def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    h = C.c_void_p()
    dummy = C.c_void_p(16)                                # never dereferenced: the arguments are checked first
    dep = np.array([0., 1., 2.])

    def create(start, nsets, nrows=10, depth=dep, out=h):
        start = np.asarray(start, dtype=np.int64)
        return lib.bh_posterior_sets_create(dummy, 0, nrows, 42, 42, None, None, start.ctypes.data, nsets,
                                            depth.ctypes.data, depth.size, None, 0, None,
                                            None if out is None else C.byref(out))
    assert create([0, 6, 4, 10], 3) == _lib.BH_ERR_ARG and b'ascending' in lib.bh_last_error() and not h.value
    assert create([0, 4, 9], 2) == _lib.BH_ERR_ARG and b'end at nrows' in lib.bh_last_error()
    assert create([1, 4, 10], 2) == _lib.BH_ERR_ARG
    assert create([0, 10], 0) == _lib.BH_ERR_ARG and b'65535' in lib.bh_last_error()
    big = np.zeros(65537, dtype=np.int64)
    big[-1] = 10
    assert create(big, 65536) == _lib.BH_ERR_ARG and b'65535' in lib.bh_last_error()
    assert create([0, 10], 1, nrows=0) == _lib.BH_ERR_ARG
    assert create([0, 10], 1, depth=np.array([0., 1., 1.])) == _lib.BH_ERR_ARG and b'ascending' in lib.bh_last_error()
    assert create([0, 10], 1, out=None) == _lib.BH_ERR_ARG
    assert lib.bh_posterior_sets_create(dummy, 0, 10, 42, 42, None, None, None, 1, dep.ctypes.data, 3, None, 0, None,
                                        C.byref(h)) == _lib.BH_ERR_ARG
    # NULL handles and outputs
    st = np.zeros(1, dtype=np.int32)
    assert lib.bh_posterior_sets_scan(None, None, None, None, None, None, None, None, st.ctypes.data) == _lib.BH_ERR_ARG
    assert lib.bh_posterior_sets_finish(None, None, None, None, 0, None, None, None) == _lib.BH_ERR_ARG
    lib.bh_posterior_sets_destroy(None)
    assert b'empty selection' in lib.bh_posterior_sets_status_text(1)
    assert b'2^53' in lib.bh_posterior_sets_status_text(2) and lib.bh_posterior_sets_status_text(0) == b''
    assert lib.bh_posterior_sets_set_chunk_bytes(None, 1 << 20) == _lib.BH_ERR_ARG


def test_summarize_sets_refuses_bad_set_start():
    from bayhunter_amd.posterior import summarize_sets
    rows = np.zeros((10, 4))
    for start in ([0, 6, 4, 10], [0, 4, 9], [1, 10], [0]):
        with pytest.raises(ValueError, match='set_start'):
            summarize_sets(rows, start, device='cpu')
