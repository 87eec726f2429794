"""GPU tier of the one-set entry points (bh_posterior_*, bh_datafits_*): they are wrappers over a sets handle with the
single set [0, nrows), and this file shows that the wrapper adds nothing.  For each reduction the one-set entry points
and the _sets entry points with set_start = [0, n] run over the same device rows, and every output -- total, excluded,
min, max, mean, std, medians / order statistics, histograms, nlayers, ifhist, argmin -- is bit for bit the same
(np.array_equal; no tolerance in this file).  What anchors the numbers themselves to numpy and to the reference's golden
files is test_gpu_posterior.py, test_gpu_datafits.py, test_gpu_scalars.py and test_gpu_moho.py.

Row counts, where the block mapping can still go wrong: 1 (a single row), 257 (two blocks, the second nearly empty), and
one row past the cap of 1 024 blocks, where the row stride exceeds one grid: 262 145 for the posterior (256 rows a
block), 32 769 for the data fits (32 row lanes a block; that is also more than the 16 384 rows one grid of the mask
kernel takes).  Posterior: float32 and float64 rows of width 42 on 9 depths (two tiles of 8), Vs edges that fit the LDS
histogram and 1 100 edges that force the global-memory one.  Data fits: 9 columns (one past the tile of 8), 3 ranks, with
and without 17 rows excluded by a NaN.

A total without statistics is where the two forms differ on purpose: the one-set scan fails with scan_fault()'s words
under its own name and leaves the handle unscanned, the sets scan reports the status of the set."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_posterior import random_rows  # noqa: E402

pytestmark = pytest.mark.gpu

DEP = np.linspace(0., 80., 9)                 # 9 depths: two tiles of 8
POST_ROWS = (1, 257, 256 * 1024 + 1)
FIT_ROWS = (1, 257, 32 * 1024 + 1)
NCOLS = 9                                     # one past the column tile of 8


def same(one, sets, path):
    """`one` (a scalar or an array) is set 0 of `sets`, bit for bit"""
    a, b = np.asarray(one), np.asarray(sets)[0]
    assert a.shape == b.shape and a.dtype == b.dtype, path
    assert np.array_equal(a, b, equal_nan=True) if a.dtype.kind == 'f' else np.array_equal(a, b), path


def test_geometry_constants_are_the_kernels():
    """the row counts above are one past the caps of the two blocks_of"""
    src = {h: open(os.path.join(ROOT, 'bayhunter_amd', 'csrc', h)).read() for h in ('posterior_kernel.h', 'datafits_kernel.h')}
    for h in src:
        assert 'constexpr int kMaxBlocksX = 1024;' in src[h] and 'constexpr int kThreads = 256;' in src[h], h
    assert 'constexpr int kCols = 8;' in src['datafits_kernel.h'] and 'kRowLanes = kThreads / kCols;' in src['datafits_kernel.h']
    assert POST_ROWS[-1] == 1024 * 256 + 1 and FIT_ROWS[-1] == 1024 * (256 // 8) + 1 and NCOLS == 8 + 1


# ---- posterior ----------------------------------------------------------------------------------------------

_post = {}


def post_rows():
    """rows of random_rows (width 42) for the largest case, a weight 0..300 each with zeros, misfits with ties"""
    if not _post:
        rs = np.random.RandomState(91)
        R = POST_ROWS[-1]
        base = random_rows(rs, 4096)
        rows = base[rs.randint(0, base.shape[0], R)]
        rows[rs.rand(R) < 0.01] = np.nan
        rows[0] = base[0]
        w = rs.randint(0, 301, R).astype(np.int32)
        w[rs.rand(R) < 0.05] = 0
        w[0] = 7
        mis = np.round(rs.uniform(1, 2, R), 2)
        for r in (255, 256, 70000, R - 1):                # the least value on both sides of block and grid boundaries
            mis[r], w[r] = 0.25, 1
        _post.update(rows=rows, w=w, mis=mis)
    return _post['rows'], _post['w'], _post['mis']


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', POST_ROWS)
def test_posterior_one_set_is_the_sets_handle_with_one_set(lib, n, dtype):
    import torch
    from bayhunter_amd.posterior import Grid, Sets, bin_index
    rows, w, mis = post_rows()
    rows, w, mis = (torch.from_numpy(np.ascontiguousarray(a[:n])).cuda() for a in (rows.astype(dtype), w, mis))
    st = torch.cuda.current_stream().cuda_stream
    dbin, ndb = bin_index(DEP, DEP), DEP.size - 1
    lds, glob = np.linspace(0.5, 5.5, 41), np.linspace(0.5, 5.5, 1100)     # 8 * 1 099 * 8 B > 64 KiB: F_HIST_GLOBAL
    with Grid(rows, w, mis, DEP, DEP, st) as one, Sets(rows, w, mis, [0, n], DEP, DEP, st) as sets:
        a, b = one.scan(), sets.scan()
        assert b['status'][0] == 0 and set(a) | {'status'} == set(b)
        for k in a:
            same(a[k], b[k], k)
        assert 0 < a['total'] <= int(w.sum()) and 0 < a['nlayers'].sum() <= a['total'] and 0 <= a['argmin'] < n
        assert a['ifhist'].size == DEP.size - 1
        for edges, stats in ((lds, True), (glob, False), (lds, True)):      # a finish leaves the handle as it found it
            ha, sa, ma = one.finish(edges, dbin, ndb, stats)
            hb, sb, mb = sets.finish([edges], dbin, ndb, stats)
            same(ha, hb, 'hist %d' % edges.size)
            assert ha.sum() > 0
            if stats:
                same(sa, sb, 'std')
                same(ma, mb, 'median')
                assert np.isfinite(sa).all() and np.isfinite(ma).all()


def test_posterior_empty_selection_is_an_error_of_the_one_set_scan_only(lib):
    import torch
    from bayhunter_amd import _lib
    from bayhunter_amd.posterior import Grid, Sets
    n = 257
    rows = torch.from_numpy(np.ascontiguousarray(post_rows()[0][:n])).cuda()
    w = torch.zeros(n, dtype=torch.int32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    with Grid(rows, w, None, DEP, None, st) as one, Sets(rows, w, None, [0, n], DEP, None, st) as sets:
        with pytest.raises(_lib.BayHunterAmdError, match=r'bh_posterior_scan: empty selection \(no included row'):
            one.scan()
        med = np.zeros(DEP.size)
        assert lib.bh_posterior_finish(one.h, None, 0, None, 0, None, None, med.ctypes.data) == _lib.BH_ERR_ARG
        assert b'bh_posterior_finish before bh_posterior_scan' in lib.bh_last_error()
        s = sets.scan()
        assert s['status'][0] == 1 and s['total'][0] == 0 and np.isnan(s['mean']).all()      # BH_POSTERIOR_SET_EMPTY
        assert lib.bh_posterior_sets_status_text(int(s['status'][0])).startswith(b'empty selection')
        w[0] = 2                                          # the caller's tensor: the next scan of the same handle succeeds
        torch.cuda.synchronize()
        a, b = one.scan(), sets.scan()
        assert a['total'] == 2 and b['status'][0] == 0
        for k in a:
            same(a[k], b[k], k)


# ---- data fits ----------------------------------------------------------------------------------------------

def fit_case(n, nnan, seed=5):
    rs = np.random.RandomState(seed)
    Y = np.round(rs.normal(0, 1, (n, NCOLS + 3)), 2)      # ties; stride > ncols
    w = rs.randint(0, 9, n).astype(np.int32)
    w[0] = 3
    bad = rs.choice(n, nnan, replace=False)
    Y[bad, rs.randint(0, NCOLS, nnan)] = np.nan
    w[bad] = np.maximum(w[bad], 1)                        # excluded by the NaN, not by the weight
    return Y, w, bad


@pytest.mark.parametrize('n,nnan', [(FIT_ROWS[0], 0), (FIT_ROWS[1], 0), (FIT_ROWS[1], 17), (FIT_ROWS[2], 17)])
def test_datafits_one_set_is_the_sets_handle_with_one_set(lib, n, nnan):
    import torch
    from bayhunter_amd.datafits import Fits, _FitsSets
    Y, w, bad = fit_case(n, nnan)
    dY, dw = torch.from_numpy(Y).cuda(), torch.from_numpy(w).cuda()
    st = torch.cuda.current_stream().cuda_stream
    with Fits(dY, NCOLS, dw, None, st) as one, _FitsSets(dY, NCOLS, dw, None, [0, n], st) as sets:
        a, b = one.scan(), sets.scan()
        assert b['status'][0] == 0 and set(a) | {'status'} == set(b)
        for k in a:
            same(np.int64(a[k]) if k in ('total', 'excluded') else a[k], b[k], k)
        ok = np.ones(n, dtype=bool)
        ok[bad] = False
        W = int(w[ok].sum())
        assert a['total'] == W > 0 and a['excluded'] == int(w[~ok].sum()) and (a['excluded'] > 0) == (nnan > 0)
        ranks = np.array([0, W // 2, W - 1], dtype=np.int64)
        eset = (np.arange(NCOLS) % 2).astype(np.int32)
        edges = np.stack([np.linspace(a['vmin'][eset == e].min() - 0.5, a['vmax'][eset == e].max() + 0.5, 12) for e in (0, 1)])
        for _ in range(2):                                # a finish leaves the handle as it found it
            oa, ha, sa = one.finish(ranks, edges, eset)
            ob, hb, sb = sets.finish(ranks[None], edges[None], eset)
            same(oa, ob, 'order statistics')
            same(ha, hb, 'hist')
            same(sa, sb, 'std')
            assert np.array_equal(oa[0], a['vmin']) and np.array_equal(oa[2], a['vmax']) and ha.sum() == W * NCOLS
            assert np.isfinite(sa).all()


@pytest.mark.parametrize('on_nan_rows', [False, True])
def test_datafits_empty_selection_still_reports_total_and_excluded(lib, on_nan_rows):
    """All weights zero, or positive on the 17 NaN rows alone: no included row with a positive weight either way."""
    import torch
    from bayhunter_amd import _lib
    n = 257
    Y, w, bad = fit_case(n, 17)
    w[:] = 0
    if on_nan_rows:
        w[bad] = 3
    dY, dw = torch.from_numpy(Y).cuda(), torch.from_numpy(w).cuda()
    start = np.array([0, n], dtype=np.int64)
    one, sets = C.c_void_p(), C.c_void_p()
    _lib.check(lib.bh_datafits_create(dY.data_ptr(), n, dY.stride(0), NCOLS, dw.data_ptr(), None, 0, None, C.byref(one)))
    try:
        _lib.check(lib.bh_datafits_sets_create(dY.data_ptr(), n, dY.stride(0), NCOLS, dw.data_ptr(), None, 0,
                                               start.ctypes.data, 1, None, C.byref(sets)))
        total, excl = C.c_longlong(-1), C.c_longlong(-1)
        assert lib.bh_datafits_scan(one, C.byref(total), C.byref(excl), None, None, None) == _lib.BH_ERR_ARG
        assert b'bh_datafits_scan: empty selection (no included row with a positive weight)' in lib.bh_last_error()
        assert total.value == 0 and excl.value == (17 * 3 if on_nan_rows else 0)
        std = np.zeros(NCOLS)
        assert lib.bh_datafits_finish(one, None, 0, None, None, 0, 0, None, None, std.ctypes.data) == _lib.BH_ERR_ARG
        assert b'bh_datafits_finish before a successful bh_datafits_scan' in lib.bh_last_error()
        tot, exc, status = np.full(1, -1, dtype=np.int64), np.full(1, -1, dtype=np.int64), np.full(1, -1, dtype=np.int32)
        _lib.check(lib.bh_datafits_sets_scan(sets, tot.ctypes.data, exc.ctypes.data, None, None, None, status.ctypes.data))
        assert status[0] == 1 and lib.bh_datafits_sets_status_text(1).startswith(b'empty selection')
        assert tot[0] == total.value and exc[0] == excl.value
    finally:
        lib.bh_datafits_destroy(one)
        lib.bh_datafits_sets_destroy(sets)
