"""GPU tier of the modelled-data statistics (bh_datafits_*, bayhunter_amd/datafits.py): the device results against
the numpy restatement (tests/datafits_ref.py) on the same modelled data, which come from ForwardEngine.run on
Model.get_vp_vs_h layers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
import datafits_ref as ref  # noqa: E402
from datafits_tolerances import STD_ATOL, STD_RTOL, check_mean, check_percentile  # noqa: E402

pytestmark = pytest.mark.gpu

Q = (2.5, 16, 50, 84, 97.5)


def make_joint(kind, rs):
    from bayhunter_amd import targets as T
    per, trf = np.linspace(1, 41, 21), np.linspace(-5, 35, 201)
    ts = []
    if kind in ('joint', 'swd75'):
        p = per if kind == 'joint' else np.linspace(1, 60, 75)
        ts.append(T.RayleighDispersionPhase(p, rs.normal(3.5, .2, p.size)))
    if kind in ('joint', 'rf'):
        ts.append(T.PReceiverFunction(trf, rs.normal(0, .05, trf.size)))
    joint = T.JointTarget(ts)
    joint.set_target_covariance([True] * len(ts), [0.0] * len(ts))
    return joint


def random_models(rs, R, maxn=8):
    rows = np.full((R, 2 * maxn), np.nan)
    n = rs.randint(2, maxn + 1, R)
    for r in range(R):
        rows[r, :n[r]] = rs.uniform(2, 5, n[r])
        rows[r, n[r]:2 * n[r]] = np.sort(rs.uniform(0, 60, n[r]))
    return rows, rs.uniform(1.6, 1.9, R)


def host_forward(joint, rows, vpvs, mantle=None):
    """Y [R, ncols] from ForwardEngine.run on host-built layers (Model.get_vp_vs_h), and each target's columns"""
    from bayhunter_amd.engine import ForwardEngine
    from bayhunter_amd.models import Model
    bl = joint.batch_layout()
    eng = ForwardEngine(swd=bl['layout'].swd, rf=bl['layout'].rf)
    R, L = rows.shape[0], rows.shape[1] // 2
    H, VP, VS = np.zeros((R, L)), np.zeros((R, L)), np.zeros((R, L))
    nl = np.zeros(R, dtype=np.int32)
    for r in range(R):
        vp, vs, h = Model.get_vp_vs_h(np.asarray(rows[r], dtype=np.float64), float(vpvs[r]), mantle)
        n = h.size
        H[r, :n], VP[r, :n], VS[r, :n], nl[r] = h, vp, vs, n
    RHO = np.where(VS > 0, VP * 0.32 + 0.77, 0.0)
    out, err = eng.run(H, VP, VS, RHO, nl)
    segs = [(bl['desc'][n].off, bl['desc'][n].off + bl['desc'][n].n) for n in range(joint.ntargets)]
    return out[:, :eng.ncols].cpu().numpy(), err.cpu().numpy(), segs


def check(res, want, segs):
    """device summarize() against the restatement"""
    assert res['nmodels'] == want['nmodels'] and res['nexcluded'] == want['nexcluded']
    for t, (a, b) in zip(res['targets'], segs):
        for k in ('min', 'max', 'median'):
            assert np.array_equal(t[k], want[k][a:b]), k
        check_percentile(t['quantiles'], want['quantiles'][:, a:b], want['lower'][:, a:b], want['upper'][:, a:b])
        np.testing.assert_allclose(t['std'], want['std'][a:b], rtol=STD_RTOL, atol=STD_ATOL)
        assert np.array_equal(t['density'][0], want['hist'][a:b])
    for t, e in zip(res['targets'], want['edges']):
        assert np.array_equal(t['density'][1], e)


def exact_equal(a, b):
    assert a['nmodels'] == b['nmodels'] and a['nexcluded'] == b['nexcluded']
    for x, y in zip(a['targets'], b['targets']):
        for k in ('min', 'max', 'median', 'quantiles'):
            assert np.array_equal(x[k], y[k]), k
        assert all(np.array_equal(p, q) for p, q in zip(x['density'], y['density']))


@pytest.mark.parametrize('kind', ['joint', 'swd75', 'rf'])
def test_summarize_against_restatement(lib, kind):
    from bayhunter_amd.datafits import summarize
    rs = np.random.RandomState({'joint': 1, 'swd75': 2, 'rf': 3}[kind])
    rows, vpvs = random_models(rs, 3000)
    w = rs.randint(0, 50, rows.shape[0]).astype(np.int32)
    joint = make_joint(kind, rs)
    Y, err, segs = host_forward(joint, rows, vpvs)
    want = ref.summarize(Y, w, Q, segs=segs, nbins=40, err=err)
    mis = rs.uniform(0, 1, rows.shape[0])
    res = summarize(joint, rows, vpvs, w, misfits=mis, nbins=40)
    check(res, want, segs)
    ok = ref.included(Y, err)
    check_mean(np.concatenate([t['mean'] for t in res['targets']]), Y[ok & (w > 0)], w[ok & (w > 0)])
    cand = np.nonzero(w > 0)[0]
    best = Y[cand[np.argmin(mis[cand])]]
    for t, (a, b) in zip(res['targets'], segs):
        assert np.array_equal(t['best'], best[a:b]) and np.array_equal(t['residual'], t['yobs'] - best[a:b])
    # the same rows expanded with weight 1, and a second call
    ex = summarize(joint, np.repeat(rows, w, axis=0), np.repeat(vpvs, w), nbins=40)
    exact_equal(res, ex)
    again = summarize(joint, rows, vpvs, w, misfits=mis, nbins=40)
    exact_equal(res, again)
    for x, y in zip(res['targets'], again['targets']):
        assert np.array_equal(x['mean'], y['mean']) and np.array_equal(x['std'], y['std'])


def fits(lib, Y, w=None, err=None, ranks=(), nbins=0, stream=None):
    """the C ABI directly on a device matrix"""
    from bayhunter_amd import _lib
    h = C.c_void_p()
    N = Y.shape[1]
    _lib.check(lib.bh_datafits_create(Y.data_ptr(), Y.shape[0], Y.stride(0), N, None if w is None else w.data_ptr(),
                                      None if err is None else err.data_ptr(), 0 if err is None else err.shape[1],
                                      stream, C.byref(h)))
    try:
        total, ex = C.c_longlong(0), C.c_longlong(0)
        vmin, vmax, mean = np.zeros(N), np.zeros(N), np.zeros(N)
        _lib.check(lib.bh_datafits_scan(h, C.byref(total), C.byref(ex), vmin.ctypes.data, vmax.ctypes.data,
                                        mean.ctypes.data))
        r = np.ascontiguousarray(ranks, dtype=np.int64)
        ost = np.zeros((max(1, r.size), N))
        hist, edges = None, None
        if nbins:
            edges = np.linspace(vmin.min(), vmax.max(), nbins + 1)[None, :]
            hist = np.zeros((N, nbins), dtype=np.int64)
        std = np.zeros(N)
        _lib.check(lib.bh_datafits_finish(h, r.ctypes.data, r.size, ost.ctypes.data,
                                          None if edges is None else edges.ctypes.data, nbins + 1, 1,
                                          np.zeros(N, dtype=np.int32).ctypes.data, None if hist is None else
                                          hist.ctypes.data, std.ctypes.data))
        if r.size:
            bad = np.array([total.value], dtype=np.int64)
            assert lib.bh_datafits_finish(h, bad.ctypes.data, 1, ost.ctypes.data, None, 0, 0, None, None,
                                          None) == _lib.BH_ERR_ARG
    finally:
        lib.bh_datafits_destroy(h)
    return dict(total=total.value, excluded=ex.value, vmin=vmin, vmax=vmax, mean=mean, ost=ost[:r.size], hist=hist,
                edges=edges, std=std)


def test_excluded_rows_are_counted(lib):
    import torch
    rs = np.random.RandomState(4)
    R, N = 20000, 37
    Y = rs.normal(0, 1, (R, N))
    Y[rs.rand(R) < 0.05, rs.randint(0, N)] = np.nan
    err = np.where(rs.rand(R, 2) < 0.03, rs.randint(1, 5, (R, 2)), 0).astype(np.int32)
    w = rs.randint(0, 9, R).astype(np.int32)
    dY = torch.from_numpy(np.concatenate((Y, np.zeros((R, 3))), axis=1)).cuda()     # stride > ncols
    res = fits(lib, dY[:, :N], torch.from_numpy(w).cuda(), torch.from_numpy(err).cuda(), ranks=[0, 5, 77], nbins=30)
    want = ref.summarize(Y, w, Q, err=err, nbins=30)
    ok = ref.included(Y, err)
    assert res['total'] == int(w[ok].sum()) and res['excluded'] == int(w[~ok].sum()) > 0
    assert np.array_equal(res['vmin'], want['min']) and np.array_equal(res['vmax'], want['max'])
    assert np.array_equal(res['ost'], ref.order_stats(Y[ok], w[ok], [0, 5, 77]))
    assert np.array_equal(res['hist'], np.stack([ref.histogram(Y[ok][:, c], w[ok], res['edges'][0])
                                                 for c in range(N)]))
    check_mean(res['mean'], Y[ok], w[ok])
    np.testing.assert_allclose(res['std'], want['std'], rtol=STD_RTOL, atol=STD_ATOL)


def test_large_weights_64bit_ranks(lib):
    import torch
    rs = np.random.RandomState(5)
    R, N = 1000000, 6
    Y = np.round(rs.normal(0, 1, (R, N)), 3)                # ties across many rows
    w = rs.randint(1, 2 ** 31 - 1, R, dtype=np.int64).astype(np.int32)
    W = int(w.astype(np.int64).sum())
    assert W > 2 ** 32
    ranks = np.unique(np.r_[0, W - 1, W // 2, (W - 1) // 2, rs.randint(0, W, 12, dtype=np.int64)])[:16]
    res = fits(lib, torch.from_numpy(Y).cuda(), torch.from_numpy(w).cuda(), ranks=ranks)
    assert res['total'] == W and res['excluded'] == 0
    assert np.array_equal(res['ost'], ref.order_stats(Y, w, ranks))


def test_lifecycle_with_own_stream(lib):
    from bayhunter_amd import _lib
    import torch
    rs = np.random.RandomState(6)
    Y = torch.from_numpy(rs.normal(0, 1, (5000, 50))).cuda()
    torch.cuda.synchronize()
    st = C.c_void_p()
    _lib.check(lib.bh_stream_create(C.byref(st)))
    res = fits(lib, Y, ranks=[2499, 2500], stream=st)
    _lib.check(lib.bh_stream_destroy(st))                     # retire + destroy
    assert res['total'] == 5000
    assert np.array_equal((res['ost'][0] + res['ost'][1]) / 2, np.median(Y.cpu().numpy(), axis=0))
    # an all-zero selection is refused
    h = C.c_void_p()
    w = torch.zeros(5000, dtype=torch.int32, device='cuda')
    _lib.check(lib.bh_datafits_create(Y.data_ptr(), 5000, 50, 50, w.data_ptr(), None, 0, None, C.byref(h)))
    assert lib.bh_datafits_scan(h, None, None, None, None, None) == _lib.BH_ERR_ARG
    lib.bh_datafits_destroy(h)


def test_finish_is_refused_after_a_failed_rescan(lib):
    from bayhunter_amd import _lib
    import torch
    rs = np.random.RandomState(7)
    Y = torch.from_numpy(rs.normal(0, 1, (3000, 20))).cuda()
    w = torch.ones(3000, dtype=torch.int32, device='cuda')
    h = C.c_void_p()
    _lib.check(lib.bh_datafits_create(Y.data_ptr(), 3000, 20, 20, w.data_ptr(), None, 0, None, C.byref(h)))
    try:
        std = np.zeros(20)
        _lib.check(lib.bh_datafits_scan(h, None, None, None, None, None))
        _lib.check(lib.bh_datafits_finish(h, None, 0, None, None, 0, 0, None, None, std.ctypes.data))
        w[17] = -1                                             # the caller's tensor: the handle reads it at every scan
        torch.cuda.synchronize()
        assert lib.bh_datafits_scan(h, None, None, None, None, None) == _lib.BH_ERR_ARG
        assert b'negative' in lib.bh_last_error()
        assert lib.bh_datafits_finish(h, None, 0, None, None, 0, 0, None, None, std.ctypes.data) == _lib.BH_ERR_ARG
        assert b'before' in lib.bh_last_error()
    finally:
        lib.bh_datafits_destroy(h)


def test_pool_datafits(lib, tmp_path):
    from chain_scenario import CASES as CH, make_pool
    from bayhunter_amd.chains import GpuEvaluator
    from bayhunter_amd.models import Model
    pool = make_pool(None, os.path.join(GOLDEN, 'tutorial_observed'), CH['tutorial'], seeds=[5, 6, 7, 8],
                     evaluator=GpuEvaluator).run()
    pool.initparams['maxmodels'] = 97
    pool.save(str(tmp_path))
    res = pool.datafits(selection='saved', exclude_outliers=False, nbins=50)
    d = tmp_path / 'data'
    chains = [i for i in range(pool.nchains) if os.path.exists(str(d / ('c%03d_p2models.npy' % i)))]
    models = np.concatenate([np.load(str(d / ('c%03d_p2models.npy' % i))) for i in chains])
    vpvs = np.concatenate([np.load(str(d / ('c%03d_p2vpvs.npy' % i))) for i in chains])
    mantle = pool.priors.get('mantle')
    Y, err, segs = host_forward(pool.targets, models, vpvs, mantle)
    check(res, ref.summarize(Y, None, Q, segs=segs, nbins=50, err=err), segs)
    assert np.array_equal(res['chains'], np.array(chains) + pool.first)
    bf = res['bestfits']
    assert np.array_equal(bf['chains'], res['chains'])
    for j, c in enumerate(chains):
        mis = np.load(str(d / ('c%03d_p2misfits.npy' % c)))
        k = int(np.argmin(mis[:, -1]))
        vp, vs, h = Model.get_vp_vs_h(np.load(str(d / ('c%03d_p2models.npy' % c)))[k].astype(np.float64),
                                      float(np.load(str(d / ('c%03d_p2vpvs.npy' % c)))[k]), mantle)
        rho = vp * 0.32 + 0.77
        for n, t in enumerate(pool.targets.targets):
            _, y = t.moddata.plugin.run_model(h, vp, vs, rho)
            assert np.array_equal(bf['data'][n][j], y), (c, t.ref)
    w = pool.datafits(selection='weighted')
    assert w['nmodels'] > res['nmodels'] and len(w['targets']) == pool.targets.ntargets
    pool.close()
