"""GPU tier of the depth-binned receiver-function sensitivity statistics (bh_rf_sens_sets_*, csrc/rf_sens_sets.hip) against
the host twin (tests/hostsim/rf_sens_sets_sim.cpp), which runs the kernel's core in the kernel's order: every output equals
the twin bit for bit, on synthetic K (random, signs mixed, NaN and 1e30 behind nlay and in the strides of K and the trace).

Sets of 0, 1, 255, 256, 257 and 513 rows and one of weight 0 in one call, Lmax = 8, nout = 80; selections of 1, 5, 27, 67
and all 80 samples (a window, every third, scattered: sample counts that are no multiple of a thread's 4 nor of a tile's
16); 1, 20 and 67 bins (cell counts that are no multiple of a tile's 64, and more than one cell tile); all four kinds;
weights 0 .. 5 and none; rows with nlay 1 and Lmax + 1; rows whose trace is NaN.  One layout at the limits (Lmax 100, 4096
samples of which 60 are selected, 1024 bins, 3 rows).  Two runs agree; a set's rows passed alone give the set's bits; rows
added in several calls cut at 256 and 512 rows from a set's first row give the bits of one call, and a cut at 100 is
refused; at 5 selected samples the result equals bh_sens_sets_* on the device bit for bit.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sens_sets_ref as ref  # noqa: E402
from test_rf_sens_sets import (FIELDS, KINDS, LMAX, NOUT, SELECTIONS, assert_same_bits, blank, load_sim, make_case, rows_of,  # noqa: E402
                               twin, view_K)

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 255, 256, 257, 513, 18]
START = np.concatenate(([0], np.cumsum(SIZES))).astype(np.int64)
GRIDS = {1: np.array([1.5, 40.]), 20: 2.5 * np.arange(21), 67: 0.5 * np.arange(68)}
_cases = {}


@pytest.fixture(scope='module')
def rsim():
    return load_sim()


def case(nan_rows=True):
    if nan_rows not in _cases:
        c = make_case(71, int(START[-1]), nan_rows=nan_rows)
        c['w'][START[1]] = 2                                # the one-row set (a built row) has weight
        c['w'][START[6]:] = 0                               # the last set has rows and no weight
        _cases[nan_rows] = c
    return _cases[nan_rows]


def device(c, start, samples, edges, kind, weights=True, cuts=(), drho=0.32, Lmax=LMAX, nout=NOUT):
    """bh_rf_sens_sets_create, one add per stretch between `cuts`, finish -> bh_rf_sens_sets_finish's arrays."""
    import torch
    from bayhunter_amd import _lib
    lib = _lib.load()
    start = np.ascontiguousarray(start, dtype=np.int64)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    smp = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32)
    Z, R, nsel = start.size - 1, c['K'].shape[0], nout if smp is None else smp.size
    if '_dev' not in c:
        c['_dev'] = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
    t = c['_dev']
    out = blank(Z, nsel, edges.size)
    h = C.c_void_p()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bh_rf_sens_sets_create(C.byref(h), start.ctypes.data, Z, nout, None if smp is None else smp.ctypes.data,
                                          nsel, edges.ctypes.data, edges.size, ref.KINDS[kind], drho, stream))
    try:
        bounds = [0] + list(cuts) + [R]
        for lo, hi in zip(bounds, bounds[1:]):
            q = t['q'][lo:hi] if kind == 'vs_total' else None
            _lib.check(lib.bh_rf_sens_sets_add(
                h, lo, hi - lo, Lmax, t['h'].shape[1], t['nlay'][lo:hi].data_ptr(), t['h'][lo:hi].data_ptr(),
                None if q is None else q.data_ptr(), 0 if q is None else t['q'].shape[1], t['K'][lo:hi].data_ptr(),
                t['K'].shape[1], t['rf'][lo:hi].data_ptr(), t['rf'].shape[1], t['w'][lo:hi].data_ptr() if weights else None))
        _lib.check(lib.bh_rf_sens_sets_finish(h, *[out[k].ctypes.data for k in FIELDS]))
    finally:
        lib.bh_rf_sens_sets_destroy(h)
    return out


def host(c):
    return {k: v for k, v in c.items() if k != '_dev'}


def assert_equal(got, want, what=''):
    for k in FIELDS:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize('nb', sorted(GRIDS))
@pytest.mark.parametrize('sel', ['one', 'window', '67'])
def test_sets_equal_the_twin_bit_for_bit(lib, rsim, sel, nb):
    c, edges, samples = case(), GRIDS[nb], SELECTIONS[sel]
    assert edges.size - 1 == nb and c['nlay'].min() == 1 and c['nlay'].max() == 9 and np.isnan(c['rf'][:, 0]).any()
    for kind in KINDS:
        want = twin(rsim, host(c), START, samples, edges, kind)
        got = device(c, START, samples, edges, kind)
        assert_equal(got, want, kind)
        assert (got['total'][[2, 3, 4, 5]] > 0).all() and not got['total'][[0, 6]].any() and got['excluded'].any()
        assert np.isnan(got['vmin'][[0, 6]]).all() and not got['s1'][[0, 6]].any() and not got['excluded'][6]
        assert np.isfinite(got['s1']).all() and np.isfinite(got['vmax'][[1, 2, 3, 4, 5]]).all()
    assert_equal(device(c, START, samples, edges, 'vs_total', weights=False),
                 twin(rsim, host(c), START, samples, edges, 'vs_total', weights=False), 'NULL')
    assert_equal(device(c, START, samples, edges, 'vs_total'), got, 'two runs')


@pytest.mark.parametrize('sel', ['all', 'third'])
def test_all_samples_and_every_third(lib, rsim, sel):
    c, edges, samples = case(), GRIDS[67], SELECTIONS[sel]
    got = device(c, START, samples, edges, 'vs_total')
    assert_equal(got, twin(rsim, host(c), START, samples, edges, 'vs_total'), sel)
    if sel == 'third':                                      # the selection picks cells of the full result
        full = device(c, START, None, edges, 'vs_total')
        for k in FIELDS[2:]:
            assert_same_bits(np.ascontiguousarray(full[k][:, samples]), got[k])


def test_a_sets_rows_alone_give_the_sets_bits(lib):
    c, edges, samples = case(), GRIDS[67], SELECTIONS['67']
    got = device(c, START, samples, edges, 'vs_total')
    for z, n in enumerate(SIZES):
        if not n:
            continue
        alone = device(rows_of(host(c), START[z], START[z + 1]), [0, n], samples, edges, 'vs_total')
        for k in FIELDS:
            assert_same_bits(alone[k][0], got[k][z])


def test_rows_added_in_several_calls_give_the_bits_of_one_call(lib):
    from bayhunter_amd import _lib
    c, edges, samples = case(), GRIDS[20], SELECTIONS['window']
    one = device(c, START, samples, edges, 'vs_total')
    first = int(START[5])                                   # the set of 513 rows
    for cuts in ((first + 256,), (first + 256, first + 512), (int(START[2]), first + 512), tuple(int(s) for s in START[1:-1])):
        assert_equal(device(c, START, samples, edges, 'vs_total', cuts=cuts), one, cuts)
    with pytest.raises(_lib.BayHunterAmdError, match='multiple of BH_SENS_SETS_BLOCK_ROWS'):
        device(c, START, samples, edges, 'vs_total', cuts=(first + 100,))
    with pytest.raises(_lib.BayHunterAmdError, match='multiple of BH_SENS_SETS_BLOCK_ROWS'):
        device(c, START, samples, edges, 'vs_total', cuts=(int(START[4]) + 256, int(START[5]) + 100))


def test_five_samples_equal_bh_sens_sets_on_the_device(lib):
    """Rows that all have a trace: bh_sens_sets_* on the same K at the 5 samples, with a finite c_out."""
    from test_gpu_sens_sets import device as sens_sets_device
    c, samples = case(nan_rows=False), SELECTIONS['window']
    h = host(c)
    other = dict(nlay=h['nlay'], h=h['h'], q=h['q'], w=h['w'], K=np.ascontiguousarray(view_K(h)[:, samples]),
                 c=np.full((h['K'].shape[0], samples.size), 3.))
    for kind in KINDS:
        for nb in (1, 67):
            got = device(c, START, samples, GRIDS[nb], kind)
            want = sens_sets_device(other, START, GRIDS[nb], kind)
            for k in FIELDS[2:]:
                assert_same_bits(got[k], want[k])
            for k in FIELDS[:2]:
                assert np.array_equal(got[k][:, None] * np.ones(samples.size, dtype=np.int64), want[k])
    assert got['total'][5] > 0 and got['excluded'][5] > 0


def test_a_negative_weight_is_reported(lib):
    from bayhunter_amd import _lib
    c = rows_of(host(case()), 0, 256)
    c['w'] = c['w'].copy()
    c['w'][17] = -1
    with pytest.raises(_lib.BayHunterAmdError, match='negative weight'):
        device(c, [0, 256], SELECTIONS['window'], GRIDS[20], 'vs_total')


def test_the_layout_at_the_limits(lib, rsim):
    """Lmax 100, 4096 samples of which 60 are selected, 1024 bins: 17 cell tiles x 4 sample tiles of one block of 3 rows."""
    rs = np.random.RandomState(77)
    Lmax, nout = 100, 4096
    K = rs.standard_normal((3, nout, 4, Lmax))
    rf = rs.standard_normal((3, nout + 1))
    c = dict(nlay=np.array([100, 37, 2], dtype=np.int32), h=rs.uniform(0.1, 1.5, (3, 103)), q=rs.uniform(1.6, 1.9, (3, 102)),
             K=np.ascontiguousarray(K.reshape(3, -1)), rf=rf, w=np.array([2, 3, 1], dtype=np.int32))
    samples = np.sort(rs.choice(nout, 60, replace=False))
    samples[0], samples[-1] = 0, nout - 1
    edges = np.linspace(0., 128., 1025)
    got = device(c, [0, 3], samples, edges, 'vs_total', Lmax=Lmax, nout=nout)
    assert_equal(got, twin(rsim, host(c), [0, 3], samples, edges, 'vs_total', Lmax=Lmax, nout=nout))
    assert got['total'][0] == 6 and got['excluded'][0] == 0
    assert np.isfinite(got['s1']).all() and (got['vmin'] <= got['vmax']).all() and got['s2'][0, :, :800].any()


def test_a_call_of_more_blocks_than_the_slab_holds(lib, rsim):
    """All 60 samples x 1025 cells are 61 500 items a block, so the slab of 64 MiB holds 34 blocks; 33 sets of one row
    and one of 300 rows are 35.  The second chunk is the last set's second block: it takes up the set's sums where the
    first chunk left them."""
    nout, Lmax, sizes = 60, 8, [1] * 33 + [300]
    edges = np.linspace(0., 128., 1025)
    assert len(sizes) + 1 == 35 > (64 << 20) // (nout * edges.size * 32)
    rs = np.random.RandomState(79)
    R = sum(sizes)
    c = dict(nlay=rs.randint(2, Lmax + 1, R).astype(np.int32), h=rs.uniform(0.2, 9., (R, Lmax + 3)),
             q=rs.uniform(1.6, 1.95, (R, Lmax + 2)), K=rs.standard_normal((R, nout * 4 * Lmax)),
             rf=rs.standard_normal((R, nout + 1)), w=rs.randint(1, 4, R).astype(np.int32))
    c['nlay'][[7, 300]] = 1, Lmax + 1                       # no model: a one-row set, and a row of the last set's second block
    start = np.concatenate(([0], np.cumsum(sizes)))
    got = device(c, start, None, edges, 'vs_total', nout=nout)
    assert_equal(got, twin(rsim, host(c), start, None, edges, 'vs_total', nout=nout))
    assert got['excluded'][7] == c['w'][7] and got['excluded'][33] == c['w'][300] and not got['total'][7]
    assert got['total'][33] == c['w'][33:].sum() - c['w'][300]
