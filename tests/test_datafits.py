"""CPU tier of the modelled-data statistics (bayhunter_amd/datafits.py, csrc/datafits.hip):

* the numpy restatement (tests/datafits_ref.py) equals numpy on the expanded matrix;
* the C ABI refuses bad arguments before it touches a device;
* the pool's best rows are what plot_bestdatafits reads from the files save() writes;
* no datafits kernel uses scratch.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import datafits_ref as ref  # noqa: E402
from datafits_tolerances import STD_ATOL, STD_RTOL, check_mean  # noqa: E402

Q = (0, 2.5, 16, 50, 84, 97.5, 100)


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_restatement_equals_numpy_on_expansion(seed):
    rs = np.random.RandomState(seed)
    R, S = rs.randint(1, 60), rs.randint(1, 9)
    Y = rs.normal(0, 1, (R, S))
    Y[:, 0] = np.round(Y[:, 0], 1)                       # ties
    w = rs.randint(0, 7, R)
    w[0] = max(w[0], 1)
    E = np.repeat(Y, w, axis=0)
    res = ref.summarize(Y, w, Q, segs=[(0, S)], nbins=13)
    assert res['nmodels'] == E.shape[0] and res['nexcluded'] == 0
    assert np.array_equal(res['quantiles'], np.percentile(E, Q, axis=0))
    assert np.array_equal(res['lower'], np.percentile(E, Q, axis=0, method='lower'))
    assert np.array_equal(res['upper'], np.percentile(E, Q, axis=0, method='higher'))
    assert np.array_equal(res['median'], np.median(E, axis=0))
    assert np.array_equal(res['min'], np.min(E, axis=0)) and np.array_equal(res['max'], np.max(E, axis=0))
    edges = res['edges'][0]
    _, want_edges = np.histogram(E, bins=13)
    assert np.array_equal(edges, want_edges)
    for c in range(S):
        assert np.array_equal(res['hist'][c], np.histogram(E[:, c], bins=edges)[0])
    check_mean(res['mean'], Y[w > 0], w[w > 0])
    np.testing.assert_allclose(res['mean'], np.mean(E, axis=0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(res['std'], np.std(E, axis=0), rtol=STD_RTOL, atol=STD_ATOL)


def test_restatement_excludes_and_widens():
    Y = np.array([[1., 2.], [np.nan, 3.], [1., 2.], [5., 6.]])
    err = np.array([[0], [0], [0], [2]])
    res = ref.summarize(Y, [1, 4, 2, 8], segs=[(0, 1), (1, 2)], nbins=4, err=err)
    assert res['nmodels'] == 3 and res['nexcluded'] == 12
    assert np.array_equal(res['edges'][0], np.histogram(np.ones(3), bins=4)[1])     # tmin == tmax: +-0.5
    assert np.array_equal(res['min'], [1., 2.])


@pytest.fixture(scope='module')
def nodev():
    return C.c_void_p(16)                  # never dereferenced: the arguments are checked first


def test_capi_refuses_bad_arguments(lib, nodev):
    from bayhunter_amd import _lib
    h = C.c_void_p()
    E = _lib.BH_ERR_ARG
    assert lib.bh_datafits_create(None, 10, 222, 222, None, None, 0, None, C.byref(h)) == E
    assert lib.bh_datafits_create(nodev, 0, 222, 222, None, None, 0, None, C.byref(h)) == E
    assert b'empty' in lib.bh_last_error()
    assert lib.bh_datafits_create(nodev, 10, 222, 0, None, None, 0, None, C.byref(h)) == E
    assert b'ncols' in lib.bh_last_error()
    assert lib.bh_datafits_create(nodev, 10, 221, 222, None, None, 0, None, C.byref(h)) == E
    assert b'stride' in lib.bh_last_error()
    assert lib.bh_datafits_create(nodev, 10, 222, 222, None, nodev, 0, None, C.byref(h)) == E
    assert lib.bh_datafits_create(nodev, (1 << 32) + 1, 222, 222, None, None, 0, None, C.byref(h)) == E
    assert not h.value
    ranks = np.arange(17, dtype=np.int64)
    out = np.zeros((17, 4))
    edges = np.array([[0., 1., 2.], [0., 2., 1.]])
    eset = np.zeros(4, dtype=np.int32)
    hist = np.zeros((4, 2), dtype=np.int64)
    fin = lambda r, n, e, ns: lib.bh_datafits_finish(None, r.ctypes.data, n, out.ctypes.data, e.ctypes.data, 3, ns,
                                                     eset.ctypes.data, hist.ctypes.data, None)
    assert fin(ranks, 17, edges, 1) == E and b'16' in lib.bh_last_error()
    neg = np.array([3, -1], dtype=np.int64)
    assert fin(neg, 2, edges, 1) == E and b'negative' in lib.bh_last_error()
    assert fin(ranks, 2, edges, 2) == E and b'ascending' in lib.bh_last_error()
    flat = np.array([[0., 1., 1.]])
    assert fin(ranks, 2, flat, 1) == E and b'ascending' in lib.bh_last_error()
    assert fin(ranks, 2, edges, 1) == E and b'NULL' in lib.bh_last_error()       # good arguments, no handle
    lib.bh_datafits_destroy(None)


@pytest.fixture(scope='module')
def pool(oracle):
    from chain_scenario import CASES as CH, make_pool
    p = make_pool(oracle, os.path.join(GOLDEN, 'tutorial_observed'), CH['fixednoise'], seeds=[5, 6, 7, 8]).run()
    p.initparams['maxmodels'] = 13                      # thinning > 1 in save()
    return p


def test_pool_best_rows_are_the_saved_argmin(pool, tmp_path):
    from bayhunter_amd.datafits import best_rows
    from bayhunter_amd.selection import pool_selection
    pool.save(str(tmp_path))
    ci, ri, w = pool_selection(pool, 'saved')
    pick = best_rows(ci, w, pool.misfits[ci, ri, -1].astype(np.float64))
    assert np.array_equal(ci[pick], np.unique(ci[w > 0]))
    d = tmp_path / 'data'
    for c, r in zip(ci[pick], ri[pick]):
        mis = np.load(str(d / ('c%03d_p2misfits.npy' % c)))
        k = int(np.argmin(mis[:, -1]))
        assert np.array_equal(np.load(str(d / ('c%03d_p2models.npy' % c)))[k], pool.models[c, r], equal_nan=True)
        assert np.load(str(d / ('c%03d_p2vpvs.npy' % c)))[k] == pool.vpvs[c, r]
        assert mis[k, -1] == pool.misfits[c, r, -1]


def test_datafits_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    r = kernel_resources('datafits.hip')                  # both forms of the handle: one kernel, three modes
    assert len([k for k in r if 'df_sets_kernel' in k]) == 3, sorted(r)
    assert all(v['scratch'] == 0 for v in r.values()), r
