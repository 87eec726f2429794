"""GPU tier of the segmented data-fit statistics (bh_datafits_sets_*), at the C ABI on synthetic matrices.

Two criteria for every set of status 0:
  * every output equals, bit for bit, what a bh_datafits handle over that set's rows alone returns (mean and std
    included): a block of df_sets_kernel runs df_block as the block it would be in df_kernel, and the slab of a set is
    added in the same order;
  * the outputs are within tests/datafits_tolerances.py of numpy on the same rows (tests/datafits_ref.py).
Shapes: the smallest at which the kernels can go wrong -- sets of 1, 31, 32, 33 rows (one block, the 32 row lanes of a
block partly filled, exactly filled, a second block) and of 32 * 1024 + 5 (the row stride of a set wraps past its 1 024
blocks), an empty segment, a set whose rows are all excluded; 1, 8, 9, 17 columns (tiles of 8: partial tiles); 1, 2, 7
sets; a chunk budget that splits the 7 sets into 4 chunks; 12 ranks that differ per set; 100 bins (LDS histogram) and
1 100 (8 * 1 100 * 8 B > 64 KiB: the global-memory histogram)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import datafits_ref as ref  # noqa: E402
from datafits_tolerances import STD_ATOL, STD_RTOL, check_mean  # noqa: E402

pytestmark = pytest.mark.gpu

NRANKS = 12
BIG = 32 * 1024 + 5


def make_case(sizes, ncols, seed, all_excluded=()):
    """Y [R, ncols + 3] (stride > ncols), w, err [R, 2], set_start: NaN values, err flags and zero weights mixed into
    every set of more than 33 rows; the sets named in all_excluded have an err flag in every row."""
    rs = np.random.RandomState(seed)
    start = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    R = int(start[-1])
    Y = np.round(rs.normal(0, 1, (R, ncols + 3)), 2)              # ties
    Y += np.repeat(np.arange(len(sizes)), sizes)[:, None] * 0.37     # every set its own range, hence its own edges
    w = rs.randint(1, 6, R).astype(np.int32)
    err = np.zeros((R, 2), dtype=np.int32)
    for z, n in enumerate(sizes):
        a, b = start[z], start[z + 1]
        if n > 33:
            Y[a + rs.choice(n, n // 20, replace=False), rs.randint(0, ncols)] = np.nan
            err[a + rs.choice(n, n // 25, replace=False), rs.randint(0, 2)] = 3
            w[a + rs.choice(n, n // 10, replace=False)] = 0
        if z in all_excluded:
            err[a:b, 1] = 1
    return Y, w, err, start


def edges_of(vmin, vmax, eset, nesets, nbins):
    out = np.zeros((nesets, nbins + 1))
    for e in range(nesets):
        lo, hi = vmin[eset == e].min(), vmax[eset == e].max()
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        out[e] = np.linspace(lo, hi, nbins + 1)
    return out


def run_sets(lib, dY, N, dw, derr, start, nbins, seed, chunk_bytes=None):
    """scan, then per-set ranks and edges made from the scan, then finish -> dict of everything"""
    from bayhunter_amd import _lib
    S = start.size - 1
    h = C.c_void_p()
    _lib.check(lib.bh_datafits_sets_create(dY.data_ptr(), dY.shape[0], dY.stride(0), N, dw.data_ptr(), derr.data_ptr(),
                                           derr.shape[1], start.ctypes.data, S, None, C.byref(h)))
    try:
        if chunk_bytes is not None:
            _lib.check(lib.bh_datafits_sets_set_chunk_bytes(h, chunk_bytes))
        std0 = np.zeros((S, N))
        assert lib.bh_datafits_sets_finish(h, None, 0, None, None, 0, 0, None, None, std0.ctypes.data) == _lib.BH_ERR_ARG
        assert b'before' in lib.bh_last_error()
        total, excl = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
        status = np.full(S, -1, dtype=np.int32)
        vmin, vmax, mean = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N))
        _lib.check(lib.bh_datafits_sets_scan(h, total.ctypes.data, excl.ctypes.data, vmin.ctypes.data, vmax.ctypes.data,
                                             mean.ctypes.data, status.ctypes.data))
        rs = np.random.RandomState(seed)
        nesets = 2 if N > 1 else 1
        eset = (np.arange(N) % nesets).astype(np.int32)
        ranks = np.zeros((S, NRANKS), dtype=np.int64)
        edges = np.zeros((S, nesets, nbins + 1))                  # a skipped set keeps zeros: they are not looked at
        for z in range(S):
            if status[z]:
                ranks[z] = -5
                continue
            W = int(total[z])
            ranks[z] = np.sort(np.r_[0, W - 1, (W - 1) // 2, W // 2, rs.randint(0, W, NRANKS - 4)])
            edges[z] = edges_of(vmin[z], vmax[z], eset, nesets, nbins)
        ost = np.zeros((S, NRANKS, N))
        hist = np.full((S, N, nbins), -1, dtype=np.int64)
        std = np.zeros((S, N))
        _lib.check(lib.bh_datafits_sets_finish(h, ranks.ctypes.data, NRANKS, ost.ctypes.data, edges.ctypes.data, nbins + 1,
                                               nesets, eset.ctypes.data, hist.ctypes.data, std.ctypes.data))
        # a rank at a live set's total is refused, before anything runs
        live = np.nonzero(status == 0)[0]
        if live.size:
            bad = ranks.copy()
            bad[live[-1], 3] = total[live[-1]]
            assert lib.bh_datafits_sets_finish(h, bad.ctypes.data, NRANKS, ost.ctypes.data, None, 0, 0, None, None,
                                               None) == _lib.BH_ERR_ARG
            assert b'rank >= the weight total' in lib.bh_last_error()
    finally:
        lib.bh_datafits_sets_destroy(h)
    return dict(total=total, excluded=excl, status=status, vmin=vmin, vmax=vmax, mean=mean, ranks=ranks, edges=edges,
                eset=eset, ost=ost, hist=hist, std=std)


def run_single(lib, dY, N, dw, derr, ranks, edges, eset):
    """a bh_datafits handle over the rows given, with the set's ranks and edges"""
    from bayhunter_amd import _lib
    h = C.c_void_p()
    _lib.check(lib.bh_datafits_create(dY.data_ptr(), dY.shape[0], dY.stride(0), N, dw.data_ptr(), derr.data_ptr(),
                                      derr.shape[1], None, C.byref(h)))
    try:
        total, ex = C.c_longlong(0), C.c_longlong(0)
        vmin, vmax, mean = np.zeros(N), np.zeros(N), np.zeros(N)
        _lib.check(lib.bh_datafits_scan(h, C.byref(total), C.byref(ex), vmin.ctypes.data, vmax.ctypes.data,
                                        mean.ctypes.data))
        ranks, edges = np.ascontiguousarray(ranks), np.ascontiguousarray(edges)
        ost = np.zeros((ranks.size, N))
        hist = np.zeros((N, edges.shape[1] - 1), dtype=np.int64)
        std = np.zeros(N)
        _lib.check(lib.bh_datafits_finish(h, ranks.ctypes.data, ranks.size, ost.ctypes.data, edges.ctypes.data,
                                          edges.shape[1], edges.shape[0], eset.ctypes.data, hist.ctypes.data,
                                          std.ctypes.data))
    finally:
        lib.bh_datafits_destroy(h)
    return dict(total=total.value, excluded=ex.value, vmin=vmin, vmax=vmax, mean=mean, ost=ost, hist=hist, std=std)


def check_case(lib, sizes, ncols, nbins, seed, chunk_bytes=None, all_excluded=()):
    import torch
    Y, w, err, start = make_case(sizes, ncols, seed, all_excluded)
    dY, dw, derr = torch.from_numpy(Y).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(err).cuda()
    got = run_sets(lib, dY, ncols, dw, derr, start, nbins, seed + 1, chunk_bytes)
    ok = ref.included(Y[:, :ncols], err)
    for z, n in enumerate(sizes):
        a, b = int(start[z]), int(start[z + 1])
        use = ok[a:b] & (w[a:b] > 0)
        assert got['excluded'][z] == int(w[a:b][~ok[a:b]].sum()), z
        if not use.any():                                          # the empty segment, the all-excluded set
            assert got['status'][z] == 1 and got['total'][z] == 0, z
            for k in ('vmin', 'vmax', 'mean', 'std', 'ost'):
                assert np.isnan(got[k][z]).all(), (z, k)
            assert not got['hist'][z].any(), z
            assert b'empty selection' in lib.bh_datafits_sets_status_text(1)
            continue
        assert got['status'][z] == 0 and got['total'][z] == int(w[a:b][use].sum()), z
        # bit for bit the single handle over the set's rows
        one = run_single(lib, dY[a:b], ncols, dw[a:b], derr[a:b], got['ranks'][z], got['edges'][z], got['eset'])
        assert one['total'] == got['total'][z] and one['excluded'] == got['excluded'][z], z
        for k in ('vmin', 'vmax', 'mean', 'ost', 'hist', 'std'):
            assert got[k][z].tobytes() == one[k].tobytes(), (z, k)
        # numpy on the same rows
        Yz, wz = Y[a:b, :ncols][use], w[a:b][use]
        assert np.array_equal(got['vmin'][z], Yz.min(axis=0)) and np.array_equal(got['vmax'][z], Yz.max(axis=0)), z
        assert np.array_equal(got['ost'][z], ref.order_stats(Yz, wz, got['ranks'][z])), z
        want_hist = np.stack([ref.histogram(Yz[:, c], wz, got['edges'][z][got['eset'][c]]) for c in range(ncols)])
        assert np.array_equal(got['hist'][z], want_hist), z
        check_mean(got['mean'][z], Yz, wz)
        wf = wz.astype(np.float64)[:, None]
        mu = (wf * Yz).sum(axis=0) / wf.sum()
        np.testing.assert_allclose(got['std'][z], np.sqrt((wf * (Yz - mu) ** 2).sum(axis=0) / wf.sum()),
                                   rtol=STD_RTOL, atol=STD_ATOL)
    return got


def test_seven_sets_in_four_chunks(lib):
    """1, 31, 32, 33 rows, an empty segment, an all-excluded set and 32 * 1024 + 5 rows; 17 columns; a digit budget of
    two sets' tables (17 columns * 12 ranks * 2 KiB each): four chunks."""
    sizes = [1, 31, 0, 32, 40, 33, BIG]
    budget = 2 * 17 * NRANKS * 2048 + 1
    got = check_case(lib, sizes, 17, 100, seed=11, chunk_bytes=budget, all_excluded=(4,))
    assert list(got['status']) == [0, 0, 1, 0, 1, 0, 0]
    # the budget changes nothing: the default takes all sets in one chunk
    again = check_case(lib, sizes, 17, 100, seed=11, all_excluded=(4,))
    for k in ('total', 'excluded', 'vmin', 'vmax', 'mean', 'ost', 'hist', 'std'):
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize('ncols,sizes', [(1, [33]), (8, [32, 70]), (9, [1, 100]), (17, [0, 65])],
                         ids=['1col_1set', '8cols_2sets', '9cols_2sets', '17cols_leading_empty'])
def test_column_tiles_and_set_counts(lib, ncols, sizes):
    check_case(lib, sizes, ncols, 100, seed=20 + ncols)


def test_histogram_in_global_memory(lib):
    """1 100 bins: 8 columns * 1 100 bins * 8 B exceed the 64 KiB of the LDS histogram"""
    check_case(lib, [33, 500], 9, 1100, seed=31)


def test_negative_weight_is_refused(lib):
    from bayhunter_amd import _lib
    import torch
    Y, w, err, start = make_case([33, 40, 70], 9, seed=41)
    w[50] = -2
    dY, dw, derr = torch.from_numpy(Y).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(err).cuda()
    h = C.c_void_p()
    _lib.check(lib.bh_datafits_sets_create(dY.data_ptr(), dY.shape[0], dY.stride(0), 9, dw.data_ptr(), derr.data_ptr(), 2,
                                           start.ctypes.data, 3, None, C.byref(h)))
    try:
        status = np.zeros(3, dtype=np.int32)
        assert lib.bh_datafits_sets_scan(h, None, None, None, None, None, status.ctypes.data) == _lib.BH_ERR_ARG
        assert b'negative weight' in lib.bh_last_error()
        std = np.zeros((3, 9))
        assert lib.bh_datafits_sets_finish(h, None, 0, None, None, 0, 0, None, None, std.ctypes.data) == _lib.BH_ERR_ARG
        assert b'before' in lib.bh_last_error()
    finally:
        lib.bh_datafits_sets_destroy(h)
