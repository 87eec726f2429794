"""GPU tier of the depth-binned sensitivity statistics (bh_sens_sets_*, csrc/sens_sets.hip) against the host twin
(tests/hostsim/sens_sets_sim.cpp), which runs the kernel's core in the kernel's order: every output equals the twin
bit for bit, on synthetic K (random, signs mixed, NaN and 1e30 behind nlay and in the strides).

Sets of 0, 1, 255, 256, 257 and 513 rows and one of weight 0 in one call -- sets start inside another set's would-be
block --, Lmax = 8, 1 and 5 periods, 1, 20 and 67 bins, all four kinds, weights 0 .. 5 and none, rows that are NaN in one
period only, rows with nlay 1 and Lmax + 1; one layout at the limits (Lmax 100, 60 periods, 1024 bins, 3 rows).  Two runs
agree; a set's rows passed alone give the set's bits; rows added in several calls cut at 256 and 512 rows from a set's
first row give the bits of one call, and a cut at 100 is refused.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sens_sets_ref as ref  # noqa: E402
from test_sens_sets import FIELDS, KINDS, assert_same_bits, load_sim, make_case, rows_of, twin  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 255, 256, 257, 513, 18]
START = np.concatenate(([0], np.cumsum(SIZES))).astype(np.int64)
GRIDS = {1: np.array([1.5, 40.]), 20: 2.5 * np.arange(21), 67: 0.5 * np.arange(68)}
_cases = {}


@pytest.fixture(scope='module')
def ssim():
    return load_sim()


def case(nper):
    if nper not in _cases:
        c = make_case(51 + nper, int(START[-1]), nper=nper)
        c['w'][START[1]] = 2                                # the one-row set (a built row) has weight
        c['w'][START[6]:] = 0                               # the last set has rows and no weight
        _cases[nper] = c
    return _cases[nper]


def device(c, start, edges, kind, weights=True, cuts=(), drho=0.32):
    """bh_sens_sets_create, one add per stretch between `cuts`, finish -> bh_sens_sets_finish's arrays."""
    import torch
    from bayhunter_amd import _lib
    lib = _lib.load()
    start = np.ascontiguousarray(start, dtype=np.int64)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    Z, (R, nper, _, Lmax) = start.size - 1, c['K'].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
    out = dict(total=np.zeros((Z, nper), dtype=np.int64), excluded=np.zeros((Z, nper), dtype=np.int64))
    for k in FIELDS[2:]:
        out[k] = np.zeros((Z, nper, edges.size))
    h = C.c_void_p()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bh_sens_sets_create(C.byref(h), start.ctypes.data, Z, nper, edges.ctypes.data, edges.size,
                                       ref.KINDS[kind], drho, stream))
    try:
        bounds = [0] + list(cuts) + [R]
        for lo, hi in zip(bounds, bounds[1:]):
            q = t['q'][lo:hi] if kind == 'vs_total' else None
            _lib.check(lib.bh_sens_sets_add(
                h, lo, hi - lo, Lmax, t['h'].shape[1], t['nlay'][lo:hi].data_ptr(), t['h'][lo:hi].data_ptr(),
                None if q is None else q.data_ptr(), 0 if q is None else t['q'].shape[1], t['K'][lo:hi].data_ptr(),
                t['c'][lo:hi].data_ptr(), t['w'][lo:hi].data_ptr() if weights else None))
        _lib.check(lib.bh_sens_sets_finish(h, *[out[k].ctypes.data for k in FIELDS]))
    finally:
        lib.bh_sens_sets_destroy(h)
    return out


def assert_equal(got, want, what=''):
    for k in FIELDS:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize('nb', sorted(GRIDS))
@pytest.mark.parametrize('nper', [1, 5])
def test_sets_equal_the_twin_bit_for_bit(lib, ssim, nper, nb):
    c, edges = case(nper), GRIDS[nb]
    assert edges.size - 1 == nb and c['nlay'].min() == 1 and c['nlay'].max() == 9 and np.isnan(c['c']).any()
    for kind in KINDS:
        want = twin(ssim, c, START, edges, kind)
        got = device(c, START, edges, kind)
        assert_equal(got, want, kind)
        assert (got['total'][[2, 3, 4, 5]] > 0).all() and not got['total'][[0, 6]].any() and got['excluded'].any()
        assert np.isnan(got['vmin'][[0, 6]]).all() and not got['s1'][[0, 6]].any() and not got['excluded'][6].any()
    assert_equal(device(c, START, edges, 'vs_total', weights=False), twin(ssim, c, START, edges, 'vs_total', weights=False), 'NULL')
    assert_equal(device(c, START, edges, 'vs_total'), got, 'two runs')


def test_a_sets_rows_alone_give_the_sets_bits(lib):
    c, edges = case(5), GRIDS[67]
    got = device(c, START, edges, 'vs_total')
    for z, n in enumerate(SIZES):
        if not n:
            continue
        alone = device(rows_of(c, START[z], START[z + 1]), [0, n], edges, 'vs_total')
        for k in FIELDS:
            assert_same_bits(alone[k][0], got[k][z])


def test_rows_added_in_several_calls_give_the_bits_of_one_call(lib):
    from bayhunter_amd import _lib
    c, edges = case(5), GRIDS[20]
    one = device(c, START, edges, 'vs_total')
    first = int(START[5])                                   # the set of 513 rows
    for cuts in ((first + 256,), (first + 256, first + 512), (int(START[2]), first + 512), tuple(int(s) for s in START[1:-1])):
        assert_equal(device(c, START, edges, 'vs_total', cuts=cuts), one, cuts)
    with pytest.raises(_lib.BayHunterAmdError, match='multiple of BH_SENS_SETS_BLOCK_ROWS'):
        device(c, START, edges, 'vs_total', cuts=(first + 100,))
    with pytest.raises(_lib.BayHunterAmdError, match='multiple of BH_SENS_SETS_BLOCK_ROWS'):
        device(c, START, edges, 'vs_total', cuts=(int(START[4]) + 256, int(START[5]) + 100))    # the end of a call inside a set


def test_the_calls_of_a_handle_are_checked(lib):
    import torch
    from bayhunter_amd import _lib
    L = _lib.load()
    c, edges = rows_of(case(5), 0, 256), GRIDS[20]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
    start = np.array([0, 256], dtype=np.int64)
    h = C.c_void_p()
    _lib.check(L.bh_sens_sets_create(C.byref(h), start.ctypes.data, 1, 5, edges.ctypes.data, edges.size, 4, 0.32, None))
    E = _lib.BH_ERR_ARG
    try:
        add = lambda row0=0, B=256, Lmax=8, ms=11, q=t['q'].data_ptr(), qs=10, w=t['w'].data_ptr(): L.bh_sens_sets_add(
            h, row0, B, Lmax, ms, t['nlay'].data_ptr(), t['h'].data_ptr(), q, qs, t['K'].data_ptr(), t['c'].data_ptr(), w)
        assert L.bh_sens_sets_finish(h, None, None, None, None, None, None) == E and b'not all rows' in L.bh_last_error()
        assert add(row0=1) == E and b'ascending order' in L.bh_last_error()
        assert add(B=257) == E and b'more rows' in L.bh_last_error()
        assert add(q=None) == E and b'needs q' in L.bh_last_error()
        assert add(qs=7) == E and add(ms=7) == E and add(Lmax=0) == E and add(Lmax=101) == E and add(B=-1) == E
        bad = t['w'].clone()
        bad[17] = -1
        assert add(w=bad.data_ptr()) == E and b'negative weight' in L.bh_last_error()
    finally:
        L.bh_sens_sets_destroy(h)


def test_the_layout_at_the_limits(lib, ssim):
    """Lmax 100, 60 periods, 1024 bins: 61 500 items in 241 groups of one block of 3 rows."""
    rs = np.random.RandomState(57)
    c = dict(nlay=np.array([100, 37, 2], dtype=np.int32), h=rs.uniform(0.1, 1.5, (3, 103)), q=rs.uniform(1.6, 1.9, (3, 102)),
             K=rs.standard_normal((3, 60, 4, 100)), c=np.full((3, 60), 3.), w=np.array([2, 3, 1], dtype=np.int32))
    c['c'][1, 7] = c['K'][1, 7] = np.nan                    # the stacks end at 80, 29 and 1 km or so
    edges = np.linspace(0., 128., 1025)
    got = device(c, [0, 3], edges, 'vs_total')
    assert_equal(got, twin(ssim, c, [0, 3], edges, 'vs_total'))
    assert got['total'][0].tolist() == [6] * 7 + [3] + [6] * 52 and got['excluded'][0, 7] == 3
    assert np.isfinite(got['s1']).all() and (got['vmin'] <= got['vmax']).all() and got['s2'][0, :, :800].any()


def test_a_call_of_more_blocks_than_the_slab_holds(lib, ssim):
    """60 periods x 1025 cells are 61 500 items a block, so the slab of 64 MiB holds 34 blocks; 33 sets of one row and
    one of 300 rows are 35.  The second chunk is the last set's second block: it takes up the set's sums where the first
    chunk left them."""
    nper, Lmax, sizes = 60, 8, [1] * 33 + [300]
    edges = np.linspace(0., 128., 1025)
    assert len(sizes) + 1 == 35 > (64 << 20) // (nper * edges.size * 32)
    rs = np.random.RandomState(59)
    R = sum(sizes)
    c = dict(nlay=rs.randint(2, Lmax + 1, R).astype(np.int32), h=rs.uniform(0.2, 9., (R, Lmax + 3)),
             q=rs.uniform(1.6, 1.95, (R, Lmax + 2)), K=rs.standard_normal((R, nper, 4, Lmax)), c=np.full((R, nper), 3.),
             w=rs.randint(1, 4, R).astype(np.int32))
    c['nlay'][[7, 300]] = 1, Lmax + 1                       # no model: a one-row set, and a row of the last set's second block
    start = np.concatenate(([0], np.cumsum(sizes)))
    got = device(c, start, edges, 'vs_total')
    assert_equal(got, twin(ssim, c, start, edges, 'vs_total'))
    assert got['excluded'][7, 0] == c['w'][7] and got['excluded'][33, 0] == c['w'][300] and not got['total'][7].any()
    assert (got['total'][33] == c['w'][33:].sum() - c['w'][300]).all()
