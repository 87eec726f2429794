"""rf_sens_kernel through bh_rf_sens_batch on the device, against the host twin (tests/hostsim/rf_sens_sim.cpp) by a
DERIVED bound, not bit equality (the device and host exponentials differ by design):

    a trace of the device lies within e = RF_TIGHT_MAX * Y * scale of the twin's (tests/tolerances.py; Y the oracle's own
    error model of tests/rf_accuracy_cases.py: the distance of the fp64 oracle from its long-double build, not below the
    batch's median; scale = max(1, max|trace|)), so the difference of two traces lies within 2 e of the twin's, and

        |K_dev - K_twin| <= 2 e / |v (1 + r) - v (1 - r)|        per entry, with no further factor.

Y is taken on the unperturbed model (the perturbed ones are 2^-17 ... 2^-20 away from it).

Shapes: B = 1, 3, 5 with ragged nlay in an Lmax = 7 batch (3, 11 and 27 slots: none a multiple of the pairs of a
workgroup; the half-space alone among them, whose trace and K are NaN), nsamp 8, 64, 256, and the smallest length at which
the launch takes the sequential form (one LDS block), with B = 1 and Lmax = 3; nout < nsamp; k_stride and rf_stride
larger than the row; both wave types.  The buffers are filled with a sentinel first: K is NaN, not stale memory, in the
layers a model does not have, and the padding behind a row stays as it was.
"""
import ctypes as C

import numpy as np
import pytest

import hp_oracle
import rf_sens_cases as rc
from tolerances import RF_TIGHT_MAX

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
NLAY = {1: [3], 3: [1, 3, 7], 5: [1, 3, 7, 2, 5]}


@pytest.fixture(scope='module')
def twin():
    return rc.load_sim()


def _models(nlay, Lmax, seed):
    from bayhunter_amd.synthetic import draw_models
    B = len(nlay)
    out = [np.zeros((B, Lmax)) for _ in range(4)]
    for b, n in enumerate(nlay):
        m = draw_models(1, max(n, 2), seed=seed + b)
        for a, x in zip(out, m[:4]):
            a[b, :n] = x[0, :n]
        out[0][b, n - 1] = 0.0
    return out


def _par(nsamp, waveno, nout):
    return dict(p=6.4, gauss=2.0, nsamp=nsamp, fsamp=5.0, tshift=min(5.0, nsamp / 25.0), nsv=None, waveno=waveno, nout=nout)


def _device(lib, models, nlay, par, k_pad=5, rf_pad=3, with_rf=True):
    """bh_rf_sens_batch on sentinel-filled buffers: (K [B][k_stride], rf [B][rf_stride], bh_rf_batch's rows [B][nout])"""
    import torch
    from bayhunter_amd import _lib
    dev = torch.device('cuda')
    B, L = models[0].shape
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in models]
    dn = torch.from_numpy(np.asarray(nlay, dtype=np.int32)).to(dev)
    nout = par['nout']
    ks, rs = nout * 4 * L + k_pad, nout + rf_pad
    K = torch.full((B, ks), SENTINEL, dtype=torch.float64, device=dev)
    rf = torch.full((B, rs), SENTINEL, dtype=torch.float64, device=dev)
    fwd = torch.full((B, nout), SENTINEL, dtype=torch.float64, device=dev)
    c = _lib.RfParams(par['p'], par['gauss'], par['fsamp'], par['tshift'], -1.0 if par['nsv'] is None else par['nsv'],
                      par['nsamp'], par['waveno'], nout, 0)
    ptr = [x.data_ptr() for x in d]
    _lib.check(lib.bh_rf_sens_batch(B, L, L, dn.data_ptr(), *ptr, None, None, C.byref(c), K.data_ptr(), ks,
                                    rf.data_ptr() if with_rf else None, rs, None, 0, None))
    _lib.check(lib.bh_rf_batch(B, L, L, dn.data_ptr(), *ptr, None, None, C.byref(c), fwd.data_ptr(), nout, None, 0, None))
    torch.cuda.synchronize()
    return K.cpu().numpy(), rf.cpu().numpy(), fwd.cpu().numpy()


def _trace_bound(models, nlay, par):
    """e [B]: RF_TIGHT_MAX * Y * scale per model (NaN for a model without a trace)"""
    from oracle import pyoracle
    B = len(nlay)
    e_ref, scale = np.full(B, np.nan), np.full(B, np.nan)
    tail = (par['p'], par['gauss'], par['nsamp'], par['fsamp'], par['tshift'], par['nsv'], par['waveno'], par['nout'])
    for b, n in enumerate(nlay):
        m = [x[b, :n] for x in models]
        O = pyoracle.rf_model(*m, *tail)
        if np.isfinite(O).all():
            X = hp_oracle.rf_model_ld(*m, *tail)
            scale[b] = max(1.0, np.abs(O).max())
            e_ref[b] = float(np.abs(O.astype(np.longdouble) - X).max()) / scale[b]
    Y = np.maximum(e_ref, np.nanmedian(e_ref))
    return RF_TIGHT_MAX * Y * scale


def _check(twin, lib, models, nlay, par):
    B, L = models[0].shape
    nout = par['nout']
    Kd, rfd, fwd = _device(lib, models, nlay, par)
    e = _trace_bound(models, nlay, par)
    steps = twin.steps()
    worst = 0.0
    for b, n in enumerate(nlay):
        Kt, _ = twin.row(*[x[b] for x in models], par, nlay=n, Lmax=L)
        K = Kd[b, :nout * 4 * L].reshape(nout, 4, L)
        assert np.all(Kd[b, nout * 4 * L:] == SENTINEL) and np.all(rfd[b, nout:] == SENTINEL)       # the padding of the rows
        assert rfd[b, :nout].tobytes() == fwd[b].tobytes()                  # the unperturbed trace: bh_rf_batch's bits
        assert np.isnan(K[:, :, n:]).all() and np.all(K[:, 0, n - 1] == 0)    # never the sentinel
        assert np.array_equal(np.isnan(K), np.isnan(Kt)), (b, n)
        if n == 1:
            assert np.isnan(K[:, 1:, 0]).all() and np.isnan(fwd[b]).all()     # a half-space alone has no trace
            continue
        assert np.isfinite(K[:, :, :n]).all() and np.isfinite(e[b])
        for k in range(4):
            v = models[k][b, :n]
            dv = np.abs(v * (1.0 + steps[k]) - v * (1.0 - steps[k]))
            live = dv > 0
            bound = 2.0 * e[b] / dv[live]
            d = np.abs(K[:, k, :n] - Kt[:, k, :n])[:, live]
            worst = max(worst, float((d / bound[None, :]).max()))
            assert np.all(d <= bound[None, :]), (b, rc.KINDS[k], float((d / bound[None, :]).max()))
            assert np.all(K[:, k, :n][:, ~live] == 0)
    print('worst |K_dev - K_twin| / bound %.4f' % worst)


@pytest.mark.parametrize('waveno', [0, 1])
@pytest.mark.parametrize('nsamp', [8, 64, 256])
@pytest.mark.parametrize('B', [1, 3, 5])
def test_device_against_the_twin_by_the_derived_bound(twin, lib, B, nsamp, waveno):
    nlay = NLAY[B]
    pairs = twin.lib.rs_pairs(7, nsamp)
    assert pairs == 4 and all((4 * n - 1) % pairs for n in nlay)           # a partial last chunk for every model
    _check(twin, lib, _models(nlay, 7, 500 + 10 * B), nlay, _par(nsamp, waveno, nsamp - 3))


@pytest.mark.parametrize('waveno', [0, 1])
def test_the_sequential_form_at_the_smallest_length_that_takes_it(twin, lib, waveno):
    lengths = [2 ** k for k in range(3, 13)]
    seq = [n for n in lengths if twin.lib.rs_pairs(3, n) == 0]
    assert seq and seq[0] == 2048 and twin.lib.rs_pairs(3, seq[0] // 2) >= 1
    assert twin.lib.rs_lds_bytes(3, seq[0]) <= 160 * 1024
    _check(twin, lib, _models([3], 3, 600), [3], _par(seq[0], waveno, seq[0] - 3))


def test_a_zero_entry_gives_zero_and_k_without_rf(twin, lib):
    models = _models([3, 5], 7, 700)
    models[3][0, 1] = 0.0                                   # a zero density: no relative step
    par = _par(64, 0, 64)
    K, rf, _ = _device(lib, models, [3, 5], par, with_rf=False)
    assert np.all(rf == SENTINEL)
    K0 = K[0, :64 * 4 * 7].reshape(64, 4, 7)
    assert np.all(K0[:, 3, 1] == 0)
    Kw, _, _ = _device(lib, models, [3, 5], par)
    assert Kw.tobytes() == K.tobytes()                      # the same launch, deterministic, with or without rf
    # nlay out of range: NaN throughout, K and rf
    Kb, rfb, fwd = _device(lib, models, [0, 8], par)
    assert np.isnan(Kb[:, :64 * 4 * 7]).all() and np.isnan(rfb[:, :64]).all() and np.isnan(fwd).all()


def test_public_paths_agree(twin, lib):
    """plugins.RFminiModRF.sensitivity, sensitivity.rf_batch and ForwardEngine.rf_sensitivity on one batch: the two batch
    paths are one launch's bits; the plugin goes through depths (thicknesses z[i+1] - z[i], a rounding away) and agrees
    within the derived bound, its trace within TOL_RF."""
    import torch
    from bayhunter_amd import plugins, sensitivity as S
    from bayhunter_amd.engine import ForwardEngine, RfSpec
    from tolerances import TOL_RF
    nlay = [3, 7, 2, 5]
    models = _models(nlay, 7, 800)
    t = np.arange(61) / 5.0 - 5.0
    for ref, waveno in (('prf', 0), ('srf', 1)):
        res = S.rf_batch(dict(obsx=t, gauss=1.5, p=5.8), *models, nlay, ref=ref)
        eng = ForwardEngine(rf=[RfSpec(ref, t, 1.5, 5.8)])
        dm = eng.upload(*models, np.asarray(nlay, dtype=np.int32))
        out, _ = eng.run(dm)
        r2 = eng.rf_sensitivity(dm)
        torch.cuda.synchronize()
        assert res['K'].shape == (4, 61, 4, 7) and res['rf'].shape == (4, 61) and np.allclose(res['t'], t)
        assert r2['K'].cpu().numpy().tobytes() == res['K'].tobytes() and r2['rf'].cpu().numpy().tobytes() == res['rf'].tobytes()
        assert out[:, eng.slices[0]].cpu().numpy().tobytes() == res['rf'].tobytes()
        plug = plugins.RFminiModRF(t, ref)
        plug.set_modelparams(gauss=1.5, p=5.8)
        par = dict(p=5.8, gauss=1.5, nsamp=int(plug.nsamp), fsamp=plug.fsamp, tshift=plug.tshft, nsv=None, waveno=waveno, nout=61)
        e = _trace_bound(models, nlay, par)
        steps = twin.steps()
        for b, n in enumerate(nlay):
            one = plug.sensitivity(*[x[b, :n] for x in models])
            _, y = plug.run_model(*[x[b, :n] for x in models])
            assert one['K'].shape == (61, 4, n) and one['rf'].tobytes() == np.asarray(y).tobytes() and np.allclose(one['t'], t)
            assert np.abs(one['rf'] - res['rf'][b]).max() <= TOL_RF
            for k in range(4):
                v = models[k][b, :n]
                dv = np.abs(v * (1.0 + steps[k]) - v * (1.0 - steps[k]))
                live = dv > 0
                d = np.abs(one['K'][:, k] - res['K'][b, :, k, :n])[:, live]
                assert np.all(d <= 2.0 * e[b] / dv[live][None, :]), (ref, b, rc.KINDS[k])
            assert np.all(one['K'][:, 0, n - 1] == 0) and np.isnan(res['K'][b, :, :, n:]).all()
