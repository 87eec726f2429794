"""CPU tier of the Moho / crustal-velocity posterior (bayhunter_amd/moho.py, csrc/moho_core.h, csrc/moho.hip):

* the per-row core, compiled with g++, equals the numpy restatement (tests/moho_ref.py) bit for bit on all four
  values, in float32 and float64: a random campaign and the built edge cases;
* the restatement's layer thicknesses are the reference's own Model.get_vp_vs_h (where the reference tree exists);
* the three C entry points refuse bad arguments before they touch a device;
* no kernel of moho.hip uses scratch and their LDS fits in 64 KiB at 50 bins.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import moho_ref as ref  # noqa: E402

WINDOW, MOHOVS = (20., 50.), 4.1
WIDTH = 40                                   # n = 1 .. 20
CAMPAIGN = 100000                            # rows per dtype: 2e5 in all
REFERENCE = '/root/reference/src'


@pytest.fixture(scope='module')
def msim():
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so = os.path.join(d, 'libmoho_sim.so')
    srcs = [os.path.join(d, 'moho_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h)
                                                for h in ('moho_core.h', 'posterior_core.h', 'stats_core.h', 'bh_common.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so, srcs[0]],
                       check=True)
    lib = C.CDLL(so)
    for f in (lib.ms_rows32, lib.ms_rows64):
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    return lib


def sim(msim, rows, moho=WINDOW, mohovs=MOHOVS):
    rows = np.ascontiguousarray(rows)
    out = np.zeros((rows.shape[0], 4))
    fn = msim.ms_rows64 if rows.dtype == np.float64 else msim.ms_rows32
    found = fn(rows.ctypes.data, rows.shape[0], rows.shape[1], rows.shape[1], moho[0], moho[1], mohovs, out.ctypes.data)
    assert found == int((~np.isnan(out[:, 0])).sum())
    return out


def assert_bits(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)])
    assert np.array_equal(np.isnan(want).all(axis=1), np.isnan(want).any(axis=1))     # four NaN or none


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_core_equals_the_restatement_on_a_random_campaign(msim, dtype):
    rs = np.random.RandomState(11 if dtype == np.float32 else 12)
    rows = ref.random_rows(rs, CAMPAIGN, WIDTH, dtype)
    n = (~np.isnan(rows)).sum(axis=1) // 2
    assert n.min() == 1 and n.max() == 20
    want = ref.derive(rows, WINDOW, MOHOVS)
    has = ~np.isnan(want[:, 0])
    assert has.mean() >= 1 / 3. and (~has).mean() >= 1 / 5., has.mean()      # the restatement alone decides
    crust = np.array([np.searchsorted(np.cumsum(ref.vs_h(r)[1]), m) + 1 for r, m in zip(rows[has][:2000], want[has][:2000, 0])])
    assert (crust >= 8).sum() > 20 and (crust < 8).sum() > 20               # both summation orders are in it
    assert_bits(sim(msim, rows), want)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_core_equals_the_restatement_on_the_built_cases(msim, dtype):
    rows, names = ref.built_cases(dtype, WIDTH, WINDOW, MOHOVS)
    want = ref.derive(rows, WINDOW, MOHOVS)
    got = sim(msim, rows)
    for i, name in enumerate(names):
        assert_bits(got[i:i + 1], want[i:i + 1]), name
    has = dict(zip(names, ~np.isnan(want[:, 0])))
    # the cases are what their names say, by the restatement
    assert not has['n1'] and has['n2'] and not has['n2 no jump'] and not has['all NaN'] and not has['window empty']
    assert not has['interface on zlo'] and not has['interface on zhi']
    assert not has['vs equal mohovs'] and has['vs one ulp above mohovs']
    for m in (7, 8, 9, 19):
        i = names.index('crust of %d' % m)
        vs, h = ref.vs_h(rows[i])
        assert has['crust of %d' % m] and want[i, 0] == np.cumsum(h)[m - 1] and want[i, 2] == vs[m - 1]
    i = names.index('two qualify')
    assert want[i, 0] == np.cumsum(ref.vs_h(rows[i])[1])[0] and abs(want[i, 0] - 25.) < 1e-4      # the shallower one
    i = names.index('velocity below an interface outside')
    assert abs(want[i, 0] - 40.) < 1e-4                     # vs[1] > mohovs lies below the 10 km interface: not it
    pairs = [i for i, nm in enumerate(names) if nm.startswith('z pair')]
    assert len(pairs) == 3 and all(~np.isnan(want[pairs, 0]))
    if dtype == np.float32:                                 # the float32 mean is not the double mean in these rows
        single = [np.float64((rows[i, 3] + rows[i, 4]) / np.float32(2)) for i in pairs]
        double = [(np.float64(rows[i, 3]) + np.float64(rows[i, 4])) / 2. for i in pairs]
        assert all(s != d for s, d in zip(single, double))
        assert all(want[i, 0] == s for i, s in zip(pairs, single))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_model_worked_by_hand(msim, dtype):
    # three layers: interfaces at 10 and 30 km, vs 3.0 / 3.5 / 4.5 -> Moho 30 km, crust (3*10 + 3.5*20) / 30
    row = ref.layered_row([3.0, 3.5, 4.5], [10., 30.], 8, dtype)
    hand = np.array([[30., (3.0 * 10 + 3.5 * 20) / 30., 3.5, 1.0]])
    assert_bits(ref.derive(row[None, :], (20., 50.), 4.2), hand)
    assert_bits(sim(msim, row[None, :], (20., 50.), 4.2), hand)
    assert np.isnan(sim(msim, row[None, :], (20., 30.), 4.2)).all()          # 30 km is not inside (20, 30)
    d = hand[0]
    res = ref.statistics(np.array([d, [np.nan] * 4, d + 1.]), [2, 3, 1], nbins=5)
    assert res['nmodels'] == 3 and res['nexcluded'] == 3 and res['moho']['median'] == 30. and res['moho']['max'] == 31.
    assert res['tradeoff']['vs_last']['counts'].sum() == 3 and res['tradeoff']['vs_last']['mode'] == pytest.approx((3.6, 30.1))


@pytest.mark.filterwarnings('ignore:invalid value')
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_moho_whose_values_hold_a_nan_is_none(msim, dtype):
    """Where the core leaves the reference on purpose.  The reference drops a model when its vs_jump is NaN (so does
    the restatement) and keeps one whose crustal mean is NaN, whose median then is NaN for the whole posterior; the
    core drops both, so that a row's four values are NaN together.  Only a window that reaches above the surface or
    infinite velocities get there."""
    width = 8
    # infinite velocities on both sides of the interface: the jump is inf - inf
    row = ref.layered_row([np.inf, np.inf, 4.5], [30., 40.], width, dtype)
    assert np.isnan(ref.derive(row[None, :], (20., 50.), 4.1)).all()
    assert np.isnan(sim(msim, row[None, :], (20., 50.), 4.1)).all()
    # nuclei at -5 and +5 km put an interface at depth 0 with no thickness above it: the crustal mean is 0 / 0
    row = np.full(width, np.nan)
    row[:2], row[2:4] = (3.0, 4.5), (-5., 5.)
    row = row.astype(dtype)
    with np.errstate(invalid='ignore'):
        want = ref.derive(row[None, :], (-1., 50.), 4.1)[0]
    assert want[0] == 0. and np.isnan(want[1]) and want[2] == 3.0 and want[3] == 1.5
    assert np.isnan(sim(msim, row[None, :], (-1., 50.), 4.1)).all()
    # the same row with the window above the surface closed has no Moho in either
    assert np.isnan(ref.derive(row[None, :], (0., 50.), 4.1)).all() and np.isnan(sim(msim, row[None, :], (0., 50.), 4.1)).all()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_crust_of_negative_zeros_sums_to_plus_zero(msim, dtype):
    """Products that are all -0: np.sum adds them to its identity 0, below and from eight terms on, and gives +0."""
    for m in (3, 8, 9, 17):
        row = ref.layered_row([-0.0] * m + [4.5], np.linspace(2., 30., m), 40, dtype)
        want = ref.derive(row[None, :], WINDOW, MOHOVS)
        assert want[0, 0] > 20. and want[0, 1] == 0. and not np.signbit(want[0, 1]) and np.signbit(want[0, 2])
        assert_bits(sim(msim, row[None, :]), want)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason='the reference tree is not on this machine')
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restatement_thicknesses_are_the_references(dtype):
    import importlib.util
    spec = importlib.util.spec_from_file_location('bayhunter_reference_models', os.path.join(REFERENCE, 'Models.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rs = np.random.RandomState(13)
    rows = np.concatenate((ref.random_rows(rs, 300, WIDTH, dtype), ref.built_cases(dtype, WIDTH, WINDOW, MOHOVS)[0]))
    for row in rows:
        if np.isnan(row).all():
            continue
        _, vs, h = mod.Model.get_vp_vs_h(row, 1.73, None)
        rvs, rh = ref.vs_h(row)
        assert h.dtype == rh.dtype == np.float64 and np.array_equal(h, rh) and np.array_equal(vs, rvs)


@pytest.fixture(scope='module')
def nodev():
    return C.c_void_p(16)                  # never dereferenced: the arguments are checked first


def test_capi_refuses_bad_arguments(lib, nodev):
    from bayhunter_amd import _lib
    E = _lib.BH_ERR_ARG
    rows = lambda *a: lib.bh_moho_rows(*a)
    assert rows(None, 0, 10, 40, 40, 20., 50., 4.2, nodev, None) == E and b'NULL' in lib.bh_last_error()
    assert rows(nodev, 0, 10, 40, 40, 20., 50., 4.2, None, None) == E
    assert rows(nodev, 0, 0, 40, 40, 20., 50., 4.2, nodev, None) == E and b'empty' in lib.bh_last_error()
    assert rows(nodev, 0, (1 << 32) + 1, 40, 40, 20., 50., 4.2, nodev, None) == E
    assert rows(nodev, 0, 10, 39, 40, 20., 50., 4.2, nodev, None) == E and b'stride' in lib.bh_last_error()
    assert rows(nodev, 0, 10, 40, 1, 20., 50., 4.2, nodev, None) == E
    assert rows(nodev, 0, 10, 400, 400, 20., 50., 4.2, nodev, None) == E
    assert rows(nodev, 0, 10, 40, 40, 50., 50., 4.2, nodev, None) == E and b'zlo < zhi' in lib.bh_last_error()
    assert rows(nodev, 0, 10, 40, 40, float('nan'), 50., 4.2, nodev, None) == E
    assert rows(nodev, 0, 10, 40, 40, 20., 50., float('nan'), nodev, None) == E and b'mohovs' in lib.bh_last_error()

    xe = np.tile(np.linspace(0., 1., 6), (3, 1))
    ye = np.linspace(0., 1., 6)
    hist = np.zeros((3, 5, 5), dtype=np.int64)
    h2 = lambda D, n, x, y, ne, h=hist: lib.bh_moho_hist2d(D, n, None, None if x is None else x.ctypes.data,
                                                            None if y is None else y.ctypes.data, ne,
                                                            None if h is None else h.ctypes.data, None)
    assert h2(None, 10, xe, ye, 6) == E and h2(nodev, 0, xe, ye, 6) == E and b'empty' in lib.bh_last_error()
    assert h2(nodev, 10, None, ye, 6) == E and h2(nodev, 10, xe, None, 6) == E and h2(nodev, 10, xe, ye, 6, None) == E
    assert h2(nodev, 10, xe, ye, 1) == E and b'edges' in lib.bh_last_error()
    bad = xe.copy()
    bad[2, 3] = bad[2, 2]
    assert h2(nodev, 10, bad, ye, 6) == E and b'ascending' in lib.bh_last_error()
    assert h2(nodev, 10, xe, ye[::-1].copy(), 6) == E and b'ascending' in lib.bh_last_error()

    out = np.zeros((3, 4))
    cnt = np.zeros(3, dtype=np.int64)
    sh = np.zeros((3, 5), dtype=np.int64)

    def sets(D, n, start, nsets, edges=ye, ne=6, h=sh):
        start = None if start is None else np.asarray(start, dtype=np.int64)
        return lib.bh_moho_sets(D, n, None, None if start is None else start.ctypes.data, nsets,
                                None if edges is None else edges.ctypes.data, ne, cnt.ctypes.data, cnt.ctypes.data,
                                out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                out.ctypes.data, None if h is None else h.ctypes.data, None)
    assert sets(None, 10, [0, 4, 10], 2) == E and sets(nodev, 0, [0, 0, 0], 2) == E
    assert sets(nodev, 10, [0, 4, 10], 0) == E and b'sets' in lib.bh_last_error()
    assert sets(nodev, 10, None, 2) == E
    assert sets(nodev, 10, [0, 6, 4, 10], 3) == E and b'ascending' in lib.bh_last_error()
    assert sets(nodev, 10, [0, 4, 9], 2) == E and b'end at nrows' in lib.bh_last_error()
    assert sets(nodev, 10, [1, 4, 10], 2) == E
    assert sets(nodev, 10, [0, 4, 10], 2, edges=ye[::-1].copy()) == E and b'ascending' in lib.bh_last_error()
    assert sets(nodev, 10, [0, 4, 10], 2, ne=1) == E
    assert sets(nodev, 10, [0, 4, 10], 2, h=None) == E


def test_python_layer_refuses_bad_arguments():
    from bayhunter_amd import moho
    rows = np.zeros((10, 4))
    for start in ([0, 6, 4, 10], [0, 4, 9], [1, 10], [0]):
        with pytest.raises(ValueError, match='set_start'):
            moho.summarize_sets(rows, start, device='cpu')
    with pytest.raises(ValueError, match='zlo < zhi'):
        moho.summarize(rows, moho=(50., 20.), device='cpu')
    with pytest.raises(ValueError, match='nbins'):
        moho.summarize(rows, moho=(20., 50.), nbins=0, device='cpu')
    assert np.array_equal(moho.outer_edges(2., 2., 4), np.histogram(np.full(3, 2.), bins=4)[1])
    assert np.array_equal(moho.outer_edges(1., 7., 50), np.histogram(np.array([1., 7.]), bins=50)[1])


def test_moho_kernels_use_no_scratch_and_fit_the_lds():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    r = kernel_resources('moho.hip')
    mine = {k: v for k, v in r.items() if 'moho_' in k}
    assert len([k for k in mine if 'moho_rows_kernel' in k]) == 2, sorted(r)
    assert len([k for k in mine if 'moho_hist2d_kernel' in k]) == 1 and len([k for k in mine if 'moho_sets_kernel' in k]) == 1
    assert all(v['scratch'] == 0 for v in r.values()), r
    nbins = 50
    dynamic = {'moho_rows_kernel': 0, 'moho_hist2d_kernel': 3 * nbins * nbins * 8, 'moho_sets_kernel': nbins * 8}
    for k, v in mine.items():
        dyn = [d for name, d in dynamic.items() if name in k][0]
        assert v['lds'] + dyn <= 64 * 1024, (k, v, dyn)
