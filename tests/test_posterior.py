"""CPU tier of the velocity-depth posterior (bayhunter_amd/posterior.py, csrc/posterior*.h/.hip):

* the numpy restatement (tests/posterior_ref.py) equals the reference's own results
  (tests/golden/posterior.npz, made by tests/golden/make_golden_posterior.py);
* the device's per-row core (posterior_core.h), compiled with g++, equals the restatement on every row and depth;
* the host side of the radix select (stats_core.h), compiled with g++ and fed numpy's digit histograms, finds
  the order statistics numpy's sort finds;
* the pool's 'weighted' / 'saved' selections are the rows weighted() / save() produce, and
  ChainPool.outliers is get_outliers on the files save() writes;
* the C ABI refuses bad arguments, and no posterior kernel uses scratch.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import posterior_ref as ref  # noqa: E402
from posterior_tolerances import MEAN_RTOL, STD_ATOL, STD_RTOL  # noqa: E402

CASES = ('default', 'deep', 'models2d')
EXACT = ('median', 'minmax', 'mode')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN, 'posterior.npz'))


def case_input(gold, case):
    dep = gold[case + '/dep_int']
    return gold['rows'], gold[case + '/weights'], (None if case == 'default' else dep), gold[case + '/misfits']


def check_against_golden(res, gold, case):
    """exact fields bit for bit, mean / std within posterior_tolerances"""
    sm = res['singlemodels']
    p = case + '/'
    assert np.array_equal(sm['median'][0], gold[p + 'median'])
    assert np.array_equal(sm['minmax'][0], gold[p + 'minmax'])
    assert np.array_equal(sm['mode'][0], gold[p + 'mode_vs']) and np.array_equal(sm['mode'][1], gold[p + 'mode_dep'])
    assert np.array_equal(sm['minmisfit'][0], gold[p + 'minmisfit_vs'])
    assert np.array_equal(sm['minmisfit'][1], gold[p + 'minmisfit_dep'])
    np.testing.assert_allclose(sm['mean'][0], gold[p + 'mean'], rtol=MEAN_RTOL, atol=0)
    gm = gold[p + 'mean']
    gstd = (gold[p + 'stdminmax'][1] - gold[p + 'stdminmax'][0]) / 2.
    std = (sm['stdminmax'][0][1] - sm['stdminmax'][0][0]) / 2.
    np.testing.assert_allclose(std, gstd, rtol=STD_RTOL, atol=STD_ATOL + 4 * MEAN_RTOL * np.abs(gm).max())
    h2, xe, ye = res['hist2d']
    assert np.array_equal(h2, gold[p + 'hist2d']) and np.array_equal(xe, gold[p + 'hist2d_vs'])
    assert np.array_equal(ye, gold[p + 'hist2d_dep'])
    assert np.array_equal(res['interfaces'][0], gold[p + 'interfaces'])
    assert np.array_equal(res['interfaces'][1], gold[p + 'interfaces_edges'])
    first = int(gold[p + 'nlayers_first']) + 1            # layers = nuclei - 1
    nl = res['nlayers'][first:first + gold[p + 'nlayers'].size]
    assert np.array_equal(nl, gold[p + 'nlayers']) and res['nlayers'].sum() == nl.sum()
    assert res['nmodels'] == int(gold[p + 'nmodels'])


@pytest.mark.parametrize('case', CASES)
def test_restatement_equals_reference_golden(gold, case):
    rows, w, dep, mis = case_input(gold, case)
    res = ref.summarize(rows, w, dep, mis)
    check_against_golden(res, gold, case)
    # the restatement's own mean is numpy's on the expanded matrix: identical, not just close
    assert np.array_equal(res['singlemodels']['mean'][0], gold[case + '/mean'])


def test_restatement_outliers_equal_reference_golden(gold, tmp_path):
    first = int(gold['outliers/first'])
    for c in range(7):
        np.save(str(tmp_path / ('c%03d_p2likes.npy' % (c + first))), gold['outliers/likes%d' % c])
    assert np.array_equal(ref.outliers_from_files(str(tmp_path)), gold['outliers/result'].astype(int))


@pytest.fixture(scope='module')
def psim():
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so = os.path.join(d, 'libposterior_sim.so')
    srcs = [os.path.join(d, 'posterior_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h)
                                                     for h in ('posterior_core.h', 'stats_core.h', 'bh_common.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so, srcs[0]],
                       check=True)
    return C.CDLL(so)


def sim_interp(psim, rows, dep):
    rows = np.ascontiguousarray(rows)
    dep = np.ascontiguousarray(dep, dtype=np.float64)
    R, W = rows.shape
    vs, n, ifd = np.zeros((R, dep.size)), np.zeros(R, dtype=np.int32), np.zeros((R, W // 2))
    fn = psim.ps_interp32 if rows.dtype == np.float32 else psim.ps_interp64
    fn(C.c_void_p(rows.ctypes.data), C.c_long(R), C.c_int(W), C.c_void_p(dep.ctypes.data), C.c_int(dep.size),
       C.c_void_p(vs.ctypes.data), C.c_void_p(n.ctypes.data), C.c_void_p(ifd.ctypes.data))
    return vs, n, ifd


def random_rows(rs, R, width=42, dtype=np.float64):
    rows = np.full((R, width), np.nan)
    n = rs.randint(1, width // 2 + 1, size=R)
    for r in range(R):
        rows[r, :n[r]] = rs.uniform(1, 5, n[r])
        z = rs.uniform(-2, 120, n[r]) if r % 5 else rs.randint(0, 60, n[r]).astype(np.float64)
        rows[r, n[r]:2 * n[r]] = np.sort(z)
    return rows.astype(dtype)


def compare_core(psim, rows, dep):
    vs, n, ifd = sim_interp(psim, rows, dep)
    valid = ~np.isnan(rows.astype(np.float64)).all(axis=1)
    want, wn, wD = ref.interp(rows[valid], dep)
    assert np.array_equal(vs[valid], want) and np.isnan(vs[~valid]).all()
    assert np.array_equal(n[valid], wn)
    W = wD.shape[1]
    assert np.array_equal(ifd[valid][:, :W], wD, equal_nan=True)


def test_core_equals_restatement_on_golden_rows(gold, psim):
    rows = gold['rows']
    for case in CASES:
        compare_core(psim, rows, gold[case + '/dep_int'])
        compare_core(psim, rows.astype(np.float64), gold[case + '/dep_int'])


def test_core_equals_restatement_on_random_rows(psim):
    rs = np.random.RandomState(5)
    dep = np.concatenate((np.linspace(-3, 100, 207), [150., 151., 400.]))
    for dtype in (np.float64, np.float32):
        compare_core(psim, random_rows(rs, 50000, dtype=dtype), dep)


def test_core_binning_and_keys(psim):
    rs = np.random.RandomState(9)
    edges = np.arange(0, 62, 1.0)
    v = np.concatenate((rs.uniform(-5, 70, 100000), edges, [np.nan, -np.inf, np.inf, 61.0]))
    out = np.zeros(v.size, dtype=np.int32)
    psim.ps_bin(C.c_void_p(edges.ctypes.data), C.c_int(edges.size), C.c_void_p(v.ctypes.data), C.c_long(v.size),
                C.c_void_p(out.ctypes.data))
    assert np.array_equal(out, ref.bin_index(v, edges))
    x = np.concatenate((rs.normal(0, 1e3, 10000), [0.0, -0.0, 1e-310, -1e-310, np.inf, -np.inf]))
    k, back = np.zeros(x.size, dtype=np.uint64), np.zeros(x.size)
    psim.ps_keys(C.c_void_p(x.ctypes.data), C.c_long(x.size), C.c_void_p(k.ctypes.data), C.c_void_p(back.ctypes.data))
    assert np.array_equal(back.view(np.uint64), x.view(np.uint64)) and np.array_equal(x[np.argsort(k)], np.sort(x))


def sim_select(psim, Y, w, ranks):
    """The 0-based `ranks` of every weighted column of Y (float64: 64-bit keys, float32: 32-bit) through
    bh::RadixSelect, numpy standing in for the device: per pass, the digit histograms of each group's keys.
    -> (values [ranks, columns], the columns' group counts of every pass)"""
    Y = np.ascontiguousarray(Y)
    R, N = Y.shape
    bits = 8 * Y.dtype.itemsize
    K, back = np.zeros(Y.size, dtype=np.uint64 if bits == 64 else np.uint32), np.zeros(Y.size, dtype=Y.dtype)
    (psim.ps_keys if bits == 64 else psim.ps_keys32)(C.c_void_p(Y.ctypes.data), C.c_long(Y.size),
                                                     C.c_void_p(K.ctypes.data), C.c_void_p(back.ctypes.data))
    K = K.reshape(R, N).astype(np.uint64)
    w = np.asarray(w).astype(np.uint64)
    ranks = np.ascontiguousarray(ranks, dtype=np.uint64)
    n = ranks.size
    psim.ps_sel_new.restype = C.c_void_p
    sel = C.c_void_p(psim.ps_sel_new(C.c_int(N), C.c_int(n), C.c_int(bits), C.c_void_p(ranks.ctypes.data)))
    gbase, ngroups, slot = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros((n, N), dtype=np.int32)
    gpfx = np.zeros(n * N, dtype=np.uint64)
    slots, maxg = C.c_int(0), C.c_int(0)
    trace = []
    try:
        while True:
            shift = psim.ps_sel_plan(sel, C.c_void_p(gbase.ctypes.data), C.c_void_p(ngroups.ctypes.data),
                                     C.c_void_p(gpfx.ctypes.data), C.c_void_p(slot.ctypes.data), C.byref(slots),
                                     C.byref(maxg))
            if shift < 0:
                break
            assert slots.value == ngroups.sum() and maxg.value == ngroups.max() and 1 <= ngroups.min()
            assert np.array_equal(gbase, np.cumsum(ngroups) - ngroups)
            for c in range(N):                                  # distinct prefixes, first occurrence in rank order
                u, first = np.unique(slot[:, c], return_index=True)
                assert np.array_equal(u, gbase[c] + np.arange(ngroups[c])) and np.all(np.diff(first) > 0)
                assert np.unique(gpfx[u]).size == u.size
            trace.append(ngroups.copy())
            digits = np.zeros((slots.value, 256), dtype=np.uint64)
            for c in range(N):
                whole = shift + 8 >= bits                       # first digit: every key matches the empty prefix
                hi = np.zeros(R, dtype=np.uint64) if whole else K[:, c] >> np.uint64(shift + 8)
                dig = ((K[:, c] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
                for t in range(ngroups[c]):
                    m = hi == gpfx[gbase[c] + t]
                    np.add.at(digits[gbase[c] + t], dig[m], w[m])
            psim.ps_sel_advance(sel, C.c_void_p(digits.ctypes.data))
        keys = np.zeros((n, N), dtype=np.uint64)
        psim.ps_sel_keys(sel, C.c_void_p(keys.ctypes.data))
    finally:
        psim.ps_sel_free(sel)
    assert len(trace) == bits // 8
    out = np.zeros((n, N), dtype=Y.dtype)
    for i in range(n):
        for c in range(N):
            at = np.nonzero((K[:, c] == keys[i, c]) & (w > 0))[0]
            assert at.size, 'rank %d of column %d: the key found is no key of the column' % (ranks[i], c)
            out[i, c] = Y[at[0], c]
    return out, trace


def sorted_order_stats(Y, w, ranks):
    """numpy's answer: the sorted values, the cumulative sum of their weights, searchsorted(side='right')"""
    out = np.zeros((len(ranks), Y.shape[1]), dtype=Y.dtype)
    for c in range(Y.shape[1]):
        o = np.argsort(Y[:, c], kind='stable')
        cum = np.cumsum(np.asarray(w, dtype=np.int64)[o])
        out[:, c] = Y[o[np.searchsorted(cum, np.asarray(ranks, dtype=np.int64), side='right')], c]
    return out


def select_ranks(rs, W, nranks):
    """ranks 0 and W - 1 first (one rank: the upper median), then the two medians, then random ones"""
    if nranks == 1:
        return np.array([W // 2], dtype=np.int64)
    if nranks == 2:
        return np.array([(W - 1) // 2, W // 2], dtype=np.int64)
    return np.r_[0, W - 1, (W - 1) // 2, W // 2, rs.randint(0, W, nranks - 4, dtype=np.int64)]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('nranks', [1, 2, 16])
def test_select_equals_numpy_sort(psim, dtype, nranks):
    rs = np.random.RandomState(100 + nranks)
    R, N = 700, 5
    Y = rs.normal(0, 3, (R, N))
    Y[:, 1] = np.round(Y[:, 1], 1)                       # duplicated values, -0.0 among them
    Y[:50, 2] = np.where(rs.rand(50) < .5, 0.0, -0.0)
    Y[:, 3] = -np.abs(Y[:, 3]) * 1e-3
    Y[:, 4] = rs.choice([-1e300, -2.5, 1e-310, 7.0, np.inf] if dtype == np.float64 else [-1e30, -2.5, 1e-40, 7.0, np.inf], R)
    Y = Y.astype(dtype)
    w = rs.randint(0, 9, R)
    W = int(w.sum())
    for ranks in (select_ranks(rs, W, nranks), np.array([0, W - 1] * 8, dtype=np.int64)[:nranks]):
        got, _ = sim_select(psim, Y, w, ranks)
        assert np.array_equal(got, np.sort(np.repeat(Y, w, axis=0), axis=0)[ranks])
        assert np.array_equal(got, sorted_order_stats(Y, w, ranks))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_select_groups_and_signed_zeros(psim, dtype):
    # one value: every rank stays in one group to the end
    Y = np.full((40, 2), 2.75, dtype=dtype)
    w = np.arange(40) % 4
    ranks = np.arange(16, dtype=np.int64) * 3
    got, trace = sim_select(psim, Y, w, ranks)
    assert np.array_equal(got, np.full((16, 2), 2.75)) and all((t == 1).all() for t in trace)
    # 16 values that differ in the first digit of their keys (sign and leading exponent bits): 16 groups from
    # the second pass on, in rank order
    step = 16 if dtype == np.float64 else 2
    v = np.r_[-(2.0 ** (step * np.arange(7, -1, -1.0))), 2.0 ** (step * np.arange(-4, 4.0))].astype(dtype)
    assert np.all(np.diff(v) > 0)
    Y = np.stack((v, v[::-1]), axis=1)
    ranks = np.array([5, 0, 15, 9, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14], dtype=np.int64)
    got, trace = sim_select(psim, Y, np.ones(16, dtype=np.int64), ranks)
    assert np.array_equal(got, np.stack((v[ranks], v[ranks]), axis=1))
    assert (trace[0] == 1).all() and all((t == 16).all() for t in trace[1:])
    # -0 sorts before +0 (the keys' order): numpy's sort cannot tell them apart, the select does
    Y = np.array([[0.0], [-0.0], [1.0], [-1.0]], dtype=dtype)
    got, _ = sim_select(psim, Y, [3, 2, 1, 1], np.arange(7))
    assert np.array_equal(got[:, 0], [-1, 0, 0, 0, 0, 0, 1])
    assert np.array_equal(np.signbit(got[:, 0]), [True, True, True, False, False, False, False])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_select_with_a_weight_total_above_2_to_32(psim, dtype):
    rs = np.random.RandomState(21)
    R = 3000
    Y = np.round(rs.normal(0, 1, (R, 3)), 2).astype(dtype)      # ties across many rows
    w = rs.randint(1, 2 ** 31 - 1, R, dtype=np.int64)
    W = int(w.sum())
    assert W > 2 ** 32
    for nranks in (2, 16):
        ranks = select_ranks(rs, W, nranks)
        got, _ = sim_select(psim, Y, w, ranks)
        assert np.array_equal(got, sorted_order_stats(Y, w, ranks))


@pytest.fixture(scope='module')
def pool(oracle):
    from chain_scenario import CASES as CH, make_pool
    p = make_pool(oracle, os.path.join(GOLDEN, 'tutorial_observed'), CH['fixednoise'], seeds=[5, 6, 7, 8]).run()
    p.initparams['maxmodels'] = 13                      # thinning > 1 in save()
    return p


def test_pool_selections_are_the_rows_weighted_and_save_produce(pool, tmp_path):
    from bayhunter_amd.selection import pool_selection
    ci, ri, w = pool_selection(pool, 'weighted')
    want = np.concatenate([pool.weighted(i)[2][0] for i in range(pool.nchains) if pool.weighted(i)[2] is not None])
    assert np.array_equal(np.repeat(pool.models[ci, ri].astype(np.float64), w, axis=0), want, equal_nan=True)
    pool.save(str(tmp_path))
    ci, ri, w = pool_selection(pool, 'saved')
    saved = np.concatenate([np.load(str(tmp_path / 'data' / ('c%03d_p2models.npy' % i))) for i in range(pool.nchains)])
    assert np.array_equal(np.repeat(pool.models[ci, ri].astype(np.float64), w, axis=0), saved, equal_nan=True)


@pytest.mark.parametrize('dev', [0.05, 0.002, 0.0005])
def test_pool_outliers_equal_get_outliers_on_saved_files(pool, tmp_path, dev):
    pool.save(str(tmp_path))
    want = ref.outliers_from_files(str(tmp_path / 'data'), dev)
    assert np.array_equal(pool.outliers(dev), want)


def test_capi_refuses_bad_arguments(lib):
    from bayhunter_amd import _lib
    h = C.c_void_p()
    dummy = C.c_void_p(16)                               # never dereferenced: the arguments are checked first
    dep = np.array([0., 1., 1., 2.])
    rc = lib.bh_posterior_create(dummy, 0, 10, 42, 42, None, None, dep.ctypes.data, dep.size, None, 0, None,
                                 C.byref(h))
    assert rc == _lib.BH_ERR_ARG and not h.value and b'ascending' in lib.bh_last_error()
    dep = np.array([0., 1., 2.])
    assert lib.bh_posterior_create(dummy, 0, 0, 42, 42, None, None, dep.ctypes.data, 3, None, 0, None,
                                   C.byref(h)) == _lib.BH_ERR_ARG
    assert lib.bh_posterior_create(dummy, 0, (1 << 32) + 1, 42, 42, None, None, dep.ctypes.data, 3, None, 0, None,
                                   C.byref(h)) == _lib.BH_ERR_ARG
    bad = np.array([0., 2., 1.])
    assert lib.bh_posterior_create(dummy, 0, 10, 42, 42, None, None, dep.ctypes.data, 3, bad.ctypes.data, 3, None,
                                   C.byref(h)) == _lib.BH_ERR_ARG
    lib.bh_posterior_destroy(None)


def test_posterior_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    r = kernel_resources('posterior.hip')                 # both forms of the handle: one kernel, float32 / float64 x scan / finish
    assert len([k for k in r if 'post_sets_kernel' in k]) == 4, sorted(r)
    assert any('sets_reduce_kernel' in k for k in r)
    assert all(v['scratch'] == 0 for v in r.values()), r


def test_host_edges_follow_the_reference():
    from bayhunter_amd import posterior
    dep = posterior.models2d_dep_int((0, 60), 1)
    d2, bins = posterior.hist_grids(dep)
    w2, wbins = ref.hist_grids(dep)
    assert np.array_equal(d2, w2) and np.array_equal(bins, wbins)
    assert np.array_equal(posterior.bin_index(d2, bins), ref.bin_index(d2, bins))
    v = np.random.RandomState(1).uniform(0, 9, 1000)
    assert np.array_equal(posterior.vs_round(v), ref.vs_round(v))
