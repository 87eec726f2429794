"""Phase-velocity sensitivity kernels on the device.

* bh_sens_batch returns, bit for bit, the host twin built with the device's math (tests/hostsim/sens_sim.cpp) -- which
  tests/test_sensitivity.py holds to the longdouble reference within tests/sensitivity_tolerances.py: Rayleigh and Love,
  batches of 1 and 65 ragged models of 2-8 layers at Lmax = 8 with garbage behind their last layer (a wave boundary in
  the model index, 32 slots per (model, period)), 1 and 5 periods, with the rows that have no value mixed in.
* Two calls give identical bits.
* bh_sensitivity and plugins.SurfDisp.sensitivity are the twin's search and pass.
* ForwardEngine.sensitivity is bh_sens_batch on the engine's own phase velocities, and refuses what is not served.
"""
import ctypes as C

import numpy as np
import pytest

import sensitivity_cases as sc

pytestmark = pytest.mark.gpu

BMAX, LMAX = 65, 8
NAMES = list(sc.MODELS)


@pytest.fixture(scope='module')
def twin():
    return sc.load_sim()


@pytest.fixture(scope='module')
def batch(twin):
    """65 ragged models ([4, 65, 8], garbage behind the last layer): the case list's models, each velocity scaled a little
    differently per row, and the phase velocities the twin's search finds -- the input both sides share."""
    rng = np.random.RandomState(11)
    M = rng.choice([np.nan, 1e30, -1.0, 0.0, 7.7], size=(4, BMAX, LMAX))            # never read
    nlay = np.zeros(BMAX, dtype=np.int32)
    C0 = {w: np.zeros((BMAX, 5)) for w in sc.WAVES}
    for b in range(BMAX):
        h, vp, vs, rho = sc.MODELS[NAMES[b % len(NAMES)]]
        s = 1.0 + 0.003 * (b // len(NAMES))
        n = nlay[b] = len(h)
        for i, x in enumerate((h, vp * s, vs * s, rho)):
            M[i, b, :n] = np.asarray(x, dtype=np.float64).astype(np.float32)
        for w in sc.WAVES:
            r = twin.sensitivity(*[M[i, b, :n] for i in range(4)], sc.PERIODS, w)
            assert r['err'] == 0
            C0[w][b] = r['c0']
    assert nlay[0] == 2 and set(nlay) == {2, 3, 4, 5, 7, 8}
    return M, nlay, C0


def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(device='cuda', dtype=dtype)


def _sens_batch(lib, M, nlay, per, wave, c, c_err, Lmax=LMAX):
    import torch
    from bayhunter_amd import _lib
    B, nper = nlay.size, per.size
    d = [_dev(M[i], torch.float64) for i in range(4)]
    dn, dper, dc, de = _dev(nlay, torch.int32), _dev(per, torch.float64), _dev(c, torch.float64), _dev(c_err, torch.int32)
    K = torch.full((B, nper, 4, Lmax), -777.0, dtype=torch.float64, device='cuda')
    co = torch.full((B, nper), -777.0, dtype=torch.float64, device='cuda')
    dT = torch.full((B, nper), -777.0, dtype=torch.float64, device='cuda')
    need = lib.bh_sens_workspace_bytes(B, nper)
    ws = torch.empty(need // 8, dtype=torch.float64, device='cuda')
    _lib.check(lib.bh_sens_batch(B, Lmax, M.shape[2], dn.data_ptr(), *[x.data_ptr() for x in d], sc.WAVES[wave], nper,
                                 dper.data_ptr(), 0, dc.data_ptr(), c.shape[1], de.data_ptr(), c_err.shape[1], K.data_ptr(),
                                 co.data_ptr(), dT.data_ptr(), ws.data_ptr(), need, None))
    torch.cuda.synchronize()
    return K.cpu().numpy(), co.cpu().numpy(), dT.cpu().numpy()


@pytest.mark.parametrize('wave', ['rayleigh', 'love'])
@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('nper', [1, 5])
def test_batch_is_the_host_twin_bit_for_bit(lib, twin, batch, wave, B, nper):
    M, nlay, C0 = batch
    M, nlay = M[:, :B].copy(), nlay[:B].copy()
    per = sc.PERIODS[:nper]
    c = np.full((B, nper + 3), 123.0)                       # a stride wider than nper; the padding is never read
    c[:, :nper] = C0[wave][:B, :nper]
    err = np.zeros((B, 2), dtype=np.int32)
    err[:, 1] = 5                                           # another target's flags
    if B > 16:                                              # the rows without a value (sensitivity_cases.NO_VALUE)
        M[2, 7, 0] = 0.0                                    # water on top
        err[8, 0], err[9, 0] = 1, 2                         # the search's flag
        c[10, 0] = 0.0                                      # c0 = 0: that period only
        c[11, nper - 1] *= 1 + 1e-5                         # c0 moved off the root: the polish is rejected
        c[12, 0] = np.nan
        nlay[13] = 1                                        # a half-space alone
        nlay[14] = LMAX + 1                                 # not a model of this batch's depth: nothing is read
    got = _sens_batch(lib, M, nlay, per, wave, c, err)
    want = [np.array(x) for x in zip(*[twin.row(*[M[i, b] for i in range(4)], per, c[b, :nper], wave, nlay=nlay[b],
                                                Lmax=LMAX, err=err[b, 0]) for b in range(B)])]
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=True)
    K, co, dT = got
    assert np.isfinite(K[0]).all() and np.all(K[0, :, :, 2:] == 0) and np.all(K[0, :, 0, 1] == 0)      # nlay = 2
    if B > 16:
        for b in (7, 8, 9, 13, 14):
            assert np.isnan(K[b]).all() and np.isnan(co[b]).all() and np.isnan(dT[b]).all(), b
        assert np.isnan(K[10, 0]).all() and np.isnan(K[11, nper - 1]).all() and np.isnan(K[12, 0]).all()
        if nper > 1:
            assert np.isfinite(K[10, 1:]).all() and np.isfinite(K[11, :nper - 1]).all()
        assert np.isfinite(K[15:]).all() and np.isfinite(co[15:]).all()
        full = np.nonzero(nlay == LMAX)[0]
        assert full.size and np.isfinite(K[full[0]]).all()                                          # nlay = Lmax
        if nper == 5:                                       # (at 3 s alone the half-space's K_vs is -0: the wave ends above it)
            assert np.all(np.any(K[full[0], :, 2, :] != 0, axis=0))                                # every layer is seen


def test_the_slot_count_is_no_multiple_of_the_wave():
    assert (65 * 5 * 4 * LMAX) % 64 != 0 and (1 * 1 * 4 * LMAX) % 64 != 0 and (65 * 4 * LMAX) % 256 != 0


def test_two_calls_give_identical_bits(lib, batch):
    M, nlay, C0 = batch
    err = np.zeros((BMAX, 1), dtype=np.int32)
    for wave in ('rayleigh', 'love'):
        a = _sens_batch(lib, M, nlay, sc.PERIODS, wave, C0[wave], err)
        b = _sens_batch(lib, M, nlay, sc.PERIODS, wave, C0[wave], err)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('wave,ref_name', [('rayleigh', 'rdispph'), ('love', 'ldispph')])
def test_single_model_forms_are_the_twins_search_and_pass(lib, twin, wave, ref_name):
    from bayhunter_amd import plugins
    for name in ('L2', 'L8', 'lvz'):
        m = sc.MODELS[name]
        want = twin.sensitivity(*m, sc.PERIODS, wave)
        f = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)) for x in m]
        n = len(f[0])
        K, c, d, err = np.zeros((5, 4, n)), np.zeros(5), np.zeros(5), C.c_int(-1)
        assert lib.bh_sensitivity(*[x.ctypes.data for x in f], n, 0, sc.WAVES[wave], 5, sc.PERIODS.ctypes.data, K.ctypes.data,
                                  c.ctypes.data, d.ctypes.data, C.byref(err)) == 0
        assert err.value == 0 and np.array_equal(K, want['K']) and np.array_equal(c, want['c']) and np.array_equal(d, want['dc_dT'])
        got = plugins.SurfDisp(sc.PERIODS, ref_name).sensitivity(*m)
        assert all(np.array_equal(got[k], want[k]) for k in ('K', 'c', 'dc_dT'))
    bad = plugins.SurfDisp(sc.PERIODS, ref_name).sensitivity([1., 0.], [np.nan, 6.], [np.nan, 3.5], [2.5, 2.8])
    assert all(np.isnan(bad[k]).all() for k in ('K', 'c', 'dc_dT'))


def test_engine_sensitivity_is_the_batch_on_the_engines_own_c(lib, batch):
    import torch
    from bayhunter_amd import sensitivity as S
    from bayhunter_amd.engine import ForwardEngine, SwdSpec
    M, nlay, _ = batch
    Mz = np.where(np.arange(LMAX)[None, None, :] < nlay[None, :, None], M, 0.0)
    eng = ForwardEngine(swd=[SwdSpec('rdispgr', sc.PERIODS), SwdSpec('ldispph', sc.PERIODS), SwdSpec('rdispph', sc.PERIODS, 2),
                             SwdSpec('rdispph', sc.PERIODS)])
    models = eng.upload(*Mz, nlay)
    out, err = eng.run(models)
    torch.cuda.synchronize()
    o, e = out.cpu().numpy(), err.cpu().numpy()
    for target, wave in ((1, 'love'), (3, 'rayleigh')):
        got = eng.sensitivity(models, out=out, err=err, target=target)
        torch.cuda.synchronize()
        sl = eng.slices[target]
        want = _sens_batch(lib, Mz, nlay, sc.PERIODS, wave, np.ascontiguousarray(o[:, sl]), np.ascontiguousarray(e[:, target:target + 1]))
        for k, w in zip(('K', 'c', 'dc_dT'), want):
            assert np.array_equal(got[k].cpu().numpy(), w, equal_nan=True)
        assert np.isfinite(want[0]).all()
        # the polished root is the engine's phase velocity to the search's tolerance
        assert np.abs(want[1] - o[:, sl]).max() <= 2e-6 * o[:, sl].max()
    with pytest.raises(ValueError, match='igr'):
        eng.sensitivity(models, out=out, err=err, target=0)
    with pytest.raises(ValueError, match='mode'):
        eng.sensitivity(models, out=out, err=err, target=2)
    # the stand-alone form: the search and the pass
    res = S.batch(sc.PERIODS, *Mz, nlay, wave='love')
    got = eng.sensitivity(models, out=out, err=err, target=1)
    assert all(np.array_equal(res[k], got[k].cpu().numpy()) for k in ('K', 'c', 'dc_dT')) and np.all(res['err'] == 0)
