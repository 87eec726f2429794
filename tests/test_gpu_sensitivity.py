"""Phase-velocity sensitivity kernels on the device.

* bh_sens_batch returns, bit for bit, the host twin built with the device's math (tests/hostsim/sens_sim.cpp) -- which
  tests/test_sensitivity.py holds to the longdouble reference within tests/sensitivity_tolerances.py: Rayleigh and Love,
  batches of 1 and 65 ragged models of 2-8 layers at Lmax = 8 with garbage behind their last layer (a wave boundary in
  the model index, 32 slots per (model, period)), 1 and 5 periods, with the rows that have no value mixed in.
* The same at every lane layout (LAYOUTS): slot counts that do not divide a wave, a (model, period) over two waves and
  over two blocks, blocks that start inside a model, 100 layers, 60 periods, strides wider than the extents with NaN,
  1e30 and set flags in the padding, rows without a value between live ones, periods at which c is a layer's vs, and a
  model whose half-space is slower than a layer above it.
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
    for name, (Lmax, nper, B, pad, _) in LAYOUTS.items():
        assert (B * nper * 4 * Lmax) % 256 != 0, name                      # the last block is partial
        if name != '8x5x6 tight':
            assert (B * nper * 4 * Lmax) % 64 != 0, name                   # and so is its last wave
    assert (4 * 5) % 64 != 0 and 64 % (4 * 5) != 0 and 4 * 17 > 64 and 4 * 100 > 256 and 7 * 4 * 10 > 256


def test_two_calls_give_identical_bits(lib, batch):
    M, nlay, C0 = batch
    err = np.zeros((BMAX, 1), dtype=np.int32)
    for wave in ('rayleigh', 'love'):
        a = _sens_batch(lib, M, nlay, sc.PERIODS, wave, C0[wave], err)
        b = _sens_batch(lib, M, nlay, sc.PERIODS, wave, C0[wave], err)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- every lane layout --------------------------------------------------------------------------------------------------------
# name -> (Lmax, nper, B, padding of the strides, rows without a value mixed in).  With 256 lanes per block and 64 per wave:
LAYOUTS = {
    '5x3x23': (5, 3, 23, 3, False),         # 20 slots: no divisor of 64; (model, period) pairs straddle waves and blocks
    '10x7x9': (10, 7, 9, 3, False),         # the benchmark's depth; 280 slots per model > 256: a block starts inside a model
    '10x7x9 mixed': (10, 7, 9, 3, True),    # ... with zero-filled rows between live ones in a block's LDS image
    '17x1x5': (17, 1, 5, 3, False),         # 68 slots: one (model, period) spans two waves
    '31x2x3': (31, 2, 3, 3, False),         # the control-paths depth, ragged
    '100x1x2': (100, 1, 2, 3, False),       # BH_MAX_LAYERS: 400 slots, a (model, period) spans two blocks, b0 == b1
    '2x60x3': (2, 60, 3, 3, False),         # the smallest depth that holds a model, at BH_MAX_PERIODS
    '2x1x70': (2, 1, 70, 3, False),         # 8 slots per model: the largest count of models in one block's LDS image
    '8x5x6 tight': (8, 5, 6, 0, False),     # the strides equal to the extents
    '8 crossing': (8, 3, 5, 3, False),      # periods at which c is the vs of a layer of L8: lanes of a wave take both branches
}
_LAYOUT_DATA = {}


def _periods_of(name, nper, wave):
    if name == '8 crossing':
        per = sorted(T for (m, w, i), T in sc.CROSSINGS.items() if m == 'L8' and w == wave)
        return [np.array(per[1:1 + nper])]                                 # row 0 is L8 itself, unscaled
    if nper == 1:
        return [np.array([3.]), np.array([30.])]                           # a short and a long period: two calls
    if nper == 60:
        return [np.geomspace(2., 60., 60)]
    return [np.geomspace(2., 40., nper)]


def _layout(twin, name, wave):
    """The models, phase velocities and the twin's rows of one layout, built once: ragged models cut from
    sensitivity_cases.MODELS by deepen(), garbage behind each row's last layer and in the strides' padding."""
    if (name, wave) in _LAYOUT_DATA:
        return _LAYOUT_DATA[(name, wave)]
    Lmax, nper, B, pad, mixed = LAYOUTS[name]
    rng = np.random.RandomState(1000 + Lmax + B)
    M = rng.choice([np.nan, 1e30, -1.0, 0.0, 7.7], size=(4, B, Lmax + pad))
    nlay = np.zeros(B, dtype=np.int32)
    fit = [n for n in NAMES if len(sc.MODELS[n][0]) <= Lmax]
    if name == '8 crossing':
        fit = ['L8', 'L3', 'lvz', 'L7', 'L8']
    for b in range(B):
        base = sc.MODELS[fit[b % len(fit)]]
        lo = len(base[0])
        n = Lmax if b == 1 else lo + (5 * b + 3 * (b // len(fit))) % (Lmax - lo + 1)
        s = 1.0 + 0.003 * (b // len(fit))
        h, vp, vs, rho = sc.deepen(base, n) if n > lo else base
        if name == '10x7x9 mixed' and b == 2:
            # a half-space slower than a layer above it: the search returns a root that is no surface wave, and the
            # pass its derivative (README): the device's bits are still the twin's
            from bayhunter_amd.synthetic import draw_models
            H, VP, VS, RHO, nl = draw_models(4, (10, 10), seed=5, sorted_vs=False)
            h, vp, vs, rho, s, n = H[0], VP[0], VS[0], RHO[0], 1.0, int(nl[0])
            assert vs[n - 1] < vs[:n].max()
        nlay[b] = n
        for i, x in enumerate((h, vp * s, vs * s, rho)):
            M[i, b, :n] = np.asarray(x, dtype=np.float64)[:n].astype(np.float32)
    assert nlay.max() == Lmax and (Lmax == 2 or len(set(nlay)) > 1)
    calls = []
    for per in _periods_of(name, nper, wave):
        c = np.tile([np.nan, 1e30, 123.0], per.size + pad)[:per.size + pad] * np.ones((B, 1))
        for b in range(B):
            r = twin.sensitivity(*[M[i, b, :nlay[b]] for i in range(4)], per, wave)
            assert r['err'] == 0 and np.all(r['c0'] > 0), (name, b)
            c[b, :per.size] = r['c0']
        err = np.zeros((B, 2 if pad else 1), dtype=np.int32)
        err[:, 1:] = 5                                                     # another target's flags
        Mc, nl = M.copy(), nlay.copy()
        if mixed:                                                          # whole rows 1, 3, 5, 7; single periods of row 4
            Mc[2, 1, 0] = 0.0                                              # water on top
            err[3, 0] = 1                                                  # the search's flag
            c[4, 0] = 0.0
            c[4, per.size - 1] *= 1 + 1e-5                                 # moved off the root
            nl[5] = 1
            nl[7] = Lmax + 1
        want = [np.array(x) for x in zip(*[twin.row(*[Mc[i, b] for i in range(4)], per, c[b, :per.size], wave, nlay=nl[b],
                                                    Lmax=Lmax, err=err[b, 0]) for b in range(B)])]
        calls.append((Mc, nl, per, c, err, want))
    _LAYOUT_DATA[(name, wave)] = calls
    return calls


def test_the_lds_image_holds_the_models_a_block_touches():
    """sens_lds_bytes reserves 255 / per_model + 2 models: the blocks of every layout touch no more (sens_kernel's b0, b1),
    2x1x70 touches the most any call can, and in 100x1x2 and 10x7x9 blocks start inside a model."""
    most = 0
    for name, (Lmax, nper, B, _, _) in LAYOUTS.items():
        per_model = nper * 4 * Lmax
        total = B * per_model
        inside = 0
        for g0 in range(0, total, 256):
            b0, b1 = g0 // per_model, min((g0 + 255) // per_model, B - 1)
            assert 1 <= b1 - b0 + 1 <= 255 // per_model + 2, name
            most = max(most, b1 - b0 + 1)
            inside += int(g0 % per_model != 0)
        assert inside or name in ('2x1x70',), name
    assert most == 256 // 8                                                # 8 slots is the fewest a model has


@pytest.mark.parametrize('wave', ['rayleigh', 'love'])
@pytest.mark.parametrize('name', list(LAYOUTS))
def test_every_layout_is_the_host_twin_bit_for_bit(lib, twin, name, wave):
    Lmax, nper, B, pad, mixed = LAYOUTS[name]
    for M, nlay, per, c, err, want in _layout(twin, name, wave):
        assert M.shape[2] == Lmax + pad and c.shape[1] == per.size + pad and err.shape[1] == (2 if pad else 1)
        got = _sens_batch(lib, M, nlay, per, wave, c, err, Lmax=Lmax)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True)
        K, co, dT = got
        if mixed:
            for b in (1, 3, 5, 7):
                assert np.isnan(K[b]).all() and np.isnan(co[b]).all() and np.isnan(dT[b]).all(), b
            assert np.isnan(K[4, 0]).all() and np.isnan(K[4, -1]).all() and np.isfinite(K[4, 1:-1]).all()
            live = [0, 2, 6, 8]                                            # each between rows whose LDS image is zeros
        else:
            live = list(range(B))
        assert np.isfinite(K[live]).all() and np.isfinite(co[live]).all() and np.isfinite(dT[live]).all()
        for b in live:
            n = nlay[b]
            assert np.all(K[b, :, :, n:] == 0) and np.all(K[b, :, 0, n - 1] == 0) and np.any(K[b, :, 2, :n] != 0)


@pytest.mark.parametrize('name', ['17x1x5', '100x1x2'])
def test_two_calls_give_identical_bits_at_depth(lib, twin, name):
    Lmax = LAYOUTS[name][0]
    for wave in ('rayleigh', 'love'):
        M, nlay, per, c, err, _ = _layout(twin, name, wave)[0]
        a = _sens_batch(lib, M, nlay, per, wave, c, err, Lmax=Lmax)
        b = _sens_batch(lib, M, nlay, per, wave, c, err, Lmax=Lmax)
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
