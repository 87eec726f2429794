"""GPU tier of the velocity-depth posterior (bh_posterior_*, bayhunter_amd/posterior.py): the device results
against the reference's golden (tests/golden/posterior.npz) and the numpy restatement (tests/posterior_ref.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import posterior_ref as ref  # noqa: E402
from posterior_tolerances import MEAN_RTOL, STD_ATOL, STD_RTOL  # noqa: E402
from test_posterior import CASES, case_input, check_against_golden, random_rows  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN, 'posterior.npz'))


def exact_equal(a, b):
    sa, sb = a['singlemodels'], b['singlemodels']
    for k in ('median', 'minmax', 'mode'):
        assert np.array_equal(sa[k][0], sb[k][0]) and np.array_equal(sa[k][1], sb[k][1]), k
    for k in ('hist2d', 'interfaces'):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
    assert np.array_equal(a['nlayers'], b['nlayers']) and a['nmodels'] == b['nmodels']


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('case', CASES)
def test_summarize_matches_reference_golden(lib, gold, case, dtype):
    from bayhunter_amd.posterior import summarize
    rows, w, dep, mis = case_input(gold, case)
    res = summarize(rows.astype(dtype), w, dep_int=dep, misfits=mis)
    check_against_golden(res, gold, case)


def test_weights_equal_expansion(lib):
    from bayhunter_amd.posterior import summarize
    rs = np.random.RandomState(11)
    rows = random_rows(rs, 200000, dtype=np.float32)
    w = rs.randint(0, 301, rows.shape[0]).astype(np.int32)
    dep = np.linspace(0, 60, 61)
    a = summarize(rows, w, dep_int=dep)
    b = summarize(np.repeat(rows, w, axis=0), dep_int=dep)
    exact_equal(a, b)
    np.testing.assert_allclose(a['singlemodels']['mean'][0], b['singlemodels']['mean'][0], rtol=MEAN_RTOL)


def test_large_counts_and_median(lib):
    from bayhunter_amd.posterior import summarize
    rs = np.random.RandomState(12)
    R = 3000000
    n = rs.randint(1, 9, R)
    rows = np.full((R, 16), np.nan, dtype=np.float32)
    vs = rs.uniform(1, 5, (R, 8)).astype(np.float32)
    z = np.sort(rs.uniform(0, 60, (R, 8)), axis=1).astype(np.float32)
    k = np.arange(8)[None, :]
    for m in range(1, 9):
        sel = n == m
        rows[sel, :m] = vs[sel, :m]
        rows[sel, m:2 * m] = z[sel, :m]
    w = rs.randint(0, 4, R).astype(np.int32)
    dep = np.linspace(0, 60, 13)
    res = summarize(rows, w, dep_int=dep)
    assert res['nmodels'] == int(w.sum()) and res['nlayers'].sum() == int(w.sum())
    assert res['hist2d'][0].sum() <= 2 * res['nmodels'] * dep.size
    vals = ref.interp(rows[w > 0], dep, chunk=65536)[0]
    want = ref.weighted_median(vals, w[w > 0].astype(np.int64))
    assert np.array_equal(res['singlemodels']['median'][0], want)
    assert k.size == 8


def test_two_calls_bit_identical(lib, gold):
    from bayhunter_amd.posterior import summarize
    rows, w, dep, mis = case_input(gold, 'deep')
    big = np.tile(rows, (300, 1))
    wb = np.tile(w, 300)
    a = summarize(big, wb, dep_int=dep)
    b = summarize(big, wb, dep_int=dep)
    exact_equal(a, b)
    for k in ('mean', 'stdminmax'):
        assert np.array_equal(a['singlemodels'][k][0], b['singlemodels'][k][0]), k


def test_pool_posterior_against_restatement(lib, tmp_path):
    from chain_scenario import CASES as CH, make_pool
    from bayhunter_amd.chains import GpuEvaluator
    pool = make_pool(None, os.path.join(GOLDEN, 'tutorial_observed'), CH['tutorial'], seeds=[5, 6, 7, 8],
                     evaluator=GpuEvaluator).run()
    pool.initparams['maxmodels'] = 97
    dep = np.arange(0, 61, 1.0)
    out = set(pool.outliers().tolist())
    res = pool.posterior(selection='weighted')
    rows = np.concatenate([pool.weighted(i)[2][0] for i in range(pool.nchains)
                           if pool.weighted(i)[2] is not None and i + pool.first not in out])
    want = ref.summarize(rows, None, dep)
    exact_equal(res, want)
    np.testing.assert_allclose(res['singlemodels']['mean'][0], want['singlemodels']['mean'][0], rtol=MEAN_RTOL)
    std = (res['singlemodels']['stdminmax'][0][1] - res['singlemodels']['stdminmax'][0][0]) / 2
    wstd = (want['singlemodels']['stdminmax'][0][1] - want['singlemodels']['stdminmax'][0][0]) / 2
    np.testing.assert_allclose(std, wstd, rtol=STD_RTOL, atol=STD_ATOL + 1e-11)
    pool.save(str(tmp_path))
    res = pool.posterior(selection='saved', exclude_outliers=False)
    saved = np.concatenate([np.load(str(tmp_path / 'data' / ('c%03d_p2models.npy' % i)))
                            for i in range(pool.nchains) if os.path.exists(str(tmp_path / 'data' / ('c%03d_p2models.npy' % i)))])
    exact_equal(res, ref.summarize(saved, None, dep))
    pool.close()


def test_lifecycle_with_own_stream(lib):
    from bayhunter_amd import _lib
    import torch
    rs = np.random.RandomState(3)
    rows = torch.from_numpy(random_rows(rs, 5000)).cuda()
    torch.cuda.synchronize()
    dep = np.linspace(0, 80, 41)
    st, h = C.c_void_p(), C.c_void_p()
    _lib.check(lib.bh_stream_create(C.byref(st)))
    _lib.check(lib.bh_posterior_create(rows.data_ptr(), 1, rows.shape[0], rows.stride(0), rows.shape[1], None, None,
                                       dep.ctypes.data, dep.size, None, 0, st, C.byref(h)))
    total = C.c_longlong(0)
    mean = np.zeros(dep.size)
    _lib.check(lib.bh_posterior_scan(h, C.byref(total), None, None, mean.ctypes.data, None, None, None))
    med = np.zeros(dep.size)
    _lib.check(lib.bh_posterior_finish(h, None, 0, None, 0, None, None, med.ctypes.data))
    lib.bh_posterior_destroy(h)
    _lib.check(lib.bh_stream_destroy(st))                     # retire + destroy
    vals = ref.interp(rows.cpu().numpy(), dep)[0]
    assert total.value == 5000 and np.array_equal(med, np.median(vals, axis=0))
    np.testing.assert_allclose(mean, vals.mean(axis=0), rtol=MEAN_RTOL)
    # an all-zero selection is refused
    w = torch.zeros(5000, dtype=torch.int32, device='cuda')
    _lib.check(lib.bh_posterior_create(rows.data_ptr(), 1, 5000, 42, 42, w.data_ptr(), None, dep.ctypes.data,
                                       dep.size, None, 0, None, C.byref(h)))
    assert lib.bh_posterior_scan(h, None, None, None, None, None, None, None) == _lib.BH_ERR_ARG
    lib.bh_posterior_destroy(h)


def test_finish_is_refused_after_a_failed_rescan(lib):
    from bayhunter_amd import _lib
    import torch
    rs = np.random.RandomState(4)
    rows = torch.from_numpy(random_rows(rs, 3000)).cuda()
    w = torch.ones(3000, dtype=torch.int32, device='cuda')
    dep = np.linspace(0, 80, 41)
    h = C.c_void_p()
    _lib.check(lib.bh_posterior_create(rows.data_ptr(), 1, 3000, rows.stride(0), rows.shape[1], w.data_ptr(), None,
                                       dep.ctypes.data, dep.size, None, 0, None, C.byref(h)))
    try:
        med = np.zeros(dep.size)
        _lib.check(lib.bh_posterior_scan(h, None, None, None, None, None, None, None))
        _lib.check(lib.bh_posterior_finish(h, None, 0, None, 0, None, None, med.ctypes.data))
        w[17] = -1                                             # the caller's tensor: the handle reads it at every scan
        torch.cuda.synchronize()
        assert lib.bh_posterior_scan(h, None, None, None, None, None, None, None) == _lib.BH_ERR_ARG
        assert b'negative' in lib.bh_last_error()
        assert lib.bh_posterior_finish(h, None, 0, None, 0, None, None, med.ctypes.data) == _lib.BH_ERR_ARG
        assert b'before' in lib.bh_last_error()
    finally:
        lib.bh_posterior_destroy(h)
