"""Rayleigh-wave ellipticity on the device.

* bh_ell_batch returns, bit for bit, the host twin built with the device's math (tests/hostsim/ell_sim.cpp) -- which
  tests/test_ellipticity.py holds to the longdouble reference within tests/ellipticity_tolerances.py: batches of 1, 63,
  65 and 130 ragged models of 2-31 layers with garbage behind their last layer, 1, 21 and 60 periods, strides wider
  than nper, rows whose c is NaN or 0 and rows whose err is set; flat and flattened earth.
* ForwardEngine with rdispph + prf + rellip: the ellipticity columns are the stand-alone call's, the dispersion and
  receiver-function columns are byte for byte those of an engine without the target, and the hidden-target layout
  gives the same ellipticities as the shared one.
* RayleighEllipticity.run_model, run_models and bh_ellipticity agree; JointTarget.evaluate values the target with the
  host likelihood.
"""
import ctypes as C

import numpy as np
import pytest

import ellipticity_cases as ec

pytestmark = pytest.mark.gpu

BMAX, LMAX = 130, 32
PER = np.linspace(1., 41., 60)


@pytest.fixture(scope='module')
def twin():
    return ec.load_sim()


def make_batch(twin):
    """130 ragged models (2-31 layers, [B, 32] with garbage behind the last layer) and the phase velocities the twin's
    search finds at PER on the flat and on the flattened earth -- the input both sides of the comparison share."""
    rng = np.random.RandomState(7)
    nlay = rng.randint(2, 32, BMAX).astype(np.int32)
    nlay[:4] = (2, 31, 3, 10)
    M = np.empty((4, BMAX, LMAX))
    M[:] = rng.choice([np.nan, 1e30, -1.0, 0.0, 7.7], size=M.shape)            # never read
    C0, C1 = np.zeros((BMAX, 60)), np.zeros((BMAX, 60))
    for b in range(BMAX):
        n = nlay[b]
        for i, x in enumerate(ec.stack(n, 100 + b, lvz=(b % 3 == 0 and n > 4))):
            M[i, b, :n] = np.asarray(x, dtype=np.float64).astype(np.float32)
        for fl, Cx in ((0, C0), (1, C1)):
            if fl == 0 or b < 65:
                _, Cx[b], err = twin.ellipticity(*[M[i, b, :n] for i in range(4)], PER, fl)
                assert err == 0
    return M, nlay, C0, C1


@pytest.fixture(scope='module')
def batch(twin):
    return make_batch(twin)


def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(device='cuda', dtype=dtype)


def _ell_batch(lib, M, nlay, per, flsph, c, c_err, absolute, out_stride, Lmax=LMAX):
    import torch
    from bayhunter_amd import _lib
    B = nlay.size
    d = [_dev(M[i], torch.float64) for i in range(4)]
    dn, dper, dc, de = _dev(nlay, torch.int32), _dev(per, torch.float64), _dev(c, torch.float64), _dev(c_err, torch.int32)
    out = torch.full((B, out_stride), -777.0, dtype=torch.float64, device='cuda')
    _lib.check(lib.bh_ell_batch(B, Lmax, M.shape[2], dn.data_ptr(), *[x.data_ptr() for x in d], per.size, dper.data_ptr(),
                                flsph, dc.data_ptr(), c.shape[1], de.data_ptr(), c_err.shape[1], 1 if absolute else 0,
                                out.data_ptr(), out_stride, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('B', [1, 63, 65, 130])
@pytest.mark.parametrize('nper', [1, 21, 60])
def test_batch_is_the_host_twin_bit_for_bit(lib, twin, batch, B, nper):
    M, nlay, C0, _ = batch
    M, nlay = M[:, :B], nlay[:B].copy()
    per = PER[:nper]
    c = np.full((B, nper + 3), 123.0)                       # strides wider than nper; the padding is never read
    c[:, :nper] = C0[:B, :nper]
    err = np.zeros((B, 2), dtype=np.int32)
    err[:, 1] = 5                                           # another target's flags
    c[0, 0] = np.nan
    if B > 8:
        c[5, nper - 1], c[6, 0], c[7, :] = 0.0, np.inf, 0.0
        err[3, 0], err[7, 0], err[8, 0] = 1, 1, 2
        nlay[9] = 1                                         # a half-space alone
        nlay[10] = LMAX + 1                                 # not a model of this batch's depth: nothing is read
    absolute = nper != 21
    got = _ell_batch(lib, M, nlay, per, 0, c, err, absolute, nper + 5)
    want = np.array([twin.row(*[M[i, b] for i in range(4)], per, c[b, :nper], nlay=nlay[b], Lmax=LMAX, err=err[b, 0],
                              absolute=absolute) for b in range(B)])
    assert np.all(got[:, nper:] == -777.0)                  # nothing written behind a row's nper values
    assert np.array_equal(got[:, :nper], want, equal_nan=True)
    assert np.isnan(want[0, 0]) and np.isfinite(want[0, 1:]).all() and np.isfinite(want[1:3]).all()
    if B > 8:
        assert np.all(np.isnan(want[[3, 7, 8, 9, 10]])) and np.isnan(want[5, nper - 1]) and np.isnan(want[6, 0])
        assert np.isfinite(want[11:]).all() and (not absolute or np.all(want[11:] > 0))


def test_flattened_earth_batch_is_the_host_twin(lib, twin, batch):
    M, nlay, _, C1 = batch
    M, nlay, c = M[:, :65], nlay[:65], C1[:65, :21].copy()
    err = np.zeros((65, 1), dtype=np.int32)
    got = _ell_batch(lib, M, nlay, PER[:21], 1, c, err, False, 21)
    want = np.array([twin.row(*[M[i, b] for i in range(4)], PER[:21], c[b], nlay=nlay[b], Lmax=LMAX, flsph=1)
                     for b in range(65)])
    flat = np.array([twin.row(*[M[i, b] for i in range(4)], PER[:21], c[b], nlay=nlay[b], Lmax=LMAX, flsph=0)
                     for b in range(65)])
    assert np.isfinite(want).all() and not np.array_equal(want, flat)
    # The flattening takes two logarithms and a power per layer and rounds the results to real*4; the device's come from
    # ocml, the twin's from the host's libm (conftest: hostsim_devmath), and where the two round a value to different
    # real*4 neighbours the layer differs by one ulp, 2^-23.  The ratio's sensitivity to a layer value is of the order of
    # its sensitivity to c, which tests/test_ellipticity.py finds at 20-30 (2e-5 .. 3e-5 for 1.1e-6): 32 x 2^-23.
    # Measured: 64 of the 65 rows bit for bit, the other (28 layers) within 3.8e-8.
    same = np.all(got == want, axis=1)
    rel = np.abs(got - want) / np.abs(want)
    print('flattened earth: %d of 65 rows bit for bit, the others within %.3e' % (same.sum(), rel.max()))
    assert same.sum() >= 0.9 * 65 and rel.max() <= 32 * 2.0 ** -23


@pytest.fixture(scope='module')
def engines():
    import torch
    from bayhunter_amd.engine import EllSpec, ForwardEngine, RfSpec, SwdSpec
    from bayhunter_amd.synthetic import draw_models
    per, t = np.linspace(1, 41, 21), np.linspace(-5, 35, 201)
    models = draw_models(96, 10, seed=3)
    res = {}
    for name, kw in (('plain', dict(swd=[SwdSpec('rdispph', per)], rf=[RfSpec('prf', t)])),
                     ('shared', dict(swd=[SwdSpec('rdispph', per)], rf=[RfSpec('prf', t)], ell=[EllSpec('rellip', per)])),
                     ('hidden', dict(rf=[RfSpec('prf', t)], ell=[EllSpec('rellip', per)])),
                     ('signed', dict(ell=[EllSpec('rellip', per, 0, False)]))):
        eng = ForwardEngine(**kw)
        out, err = eng.run(*models)
        torch.cuda.synchronize()
        res[name] = (eng, out.cpu().numpy(), err.cpu().numpy())
    return per, models, res


def test_engine_columns(lib, engines):
    per, (H, VP, VS, RHO, nl), res = engines
    plain, shared, hidden, signed = (res[k] for k in ('plain', 'shared', 'hidden', 'signed'))
    eng = shared[0]
    assert eng.slices == [slice(0, 21), slice(21, 222), slice(222, 243)] and eng.row == 243 and shared[2].shape == (96, 1)
    assert hidden[0].slices == [slice(0, 201), slice(201, 222)] and hidden[0].row == 243 and hidden[2].shape == (96, 1)
    # the dispersion and receiver-function columns do not know about the new target
    assert shared[1][:, :222].tobytes() == plain[1][:, :222].tobytes() and np.array_equal(shared[2], plain[2])
    assert hidden[1][:, :201].tobytes() == plain[1][:, 21:222].tobytes() and np.array_equal(hidden[2], plain[2])
    assert hidden[1][:, 222:243].tobytes() == plain[1][:, :21].tobytes()        # the hidden target's phase velocities
    # the ellipticity columns are the stand-alone call on the engine's own phase velocities
    M = np.stack([H, VP, VS, RHO])
    alone = _ell_batch(lib, M, np.asarray(nl, dtype=np.int32), per, 0, np.ascontiguousarray(plain[1][:, :21]),
                       np.ascontiguousarray(plain[2][:, :1]), True, 21, Lmax=M.shape[2])
    assert np.array_equal(shared[1][:, 222:], alone, equal_nan=True)
    assert np.array_equal(hidden[1][:, 201:222], alone, equal_nan=True)
    assert np.array_equal(np.abs(signed[1][:, :21]), alone, equal_nan=True)
    ok = plain[2][:, 0] == 0
    assert ok.sum() > 80 and np.isfinite(alone[ok]).all() and np.all(alone[ok] > 0) and np.isnan(alone[~ok]).all()
    assert np.all((alone[ok] > 0.3) & (alone[ok] < 3.0))                      # crustal models: H/V of order one


def test_plugin_forms_agree(lib, engines):
    from bayhunter_amd import plugins
    per, (H, VP, VS, RHO, nl), res = engines
    p = plugins.RayleighEllipticity(per)
    x, Y, flags = p.run_models(H, VP, VS, RHO, nl)
    assert np.array_equal(x, per) and np.array_equal(Y, res['shared'][1][:, 222:], equal_nan=True)
    assert np.array_equal(flags, res['plain'][2][:, 0])
    for b in range(6):
        n = int(nl[b])
        xm, ym = p.run_model(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n])
        f = [np.ascontiguousarray(a[b, :n].astype(np.float32)) for a in (H, VP, VS, RHO)]
        ell, err = np.zeros(21), C.c_int(-1)
        assert lib.bh_ellipticity(*[a.ctypes.data for a in f], n, 0, 21, per.ctypes.data, 1, ell.ctypes.data,
                                  C.byref(err)) == 0
        if flags[b] != 0:
            assert err.value != 0 and np.isnan(ell).all() and np.isnan(xm) and np.isnan(ym)
        else:
            assert err.value == 0 and np.array_equal(xm, per) and np.array_equal(ym, Y[b]) and np.array_equal(ell, Y[b])
    # the signed form, and a water layer on top: no ellipticity
    (h, vp, vs, rho), per60 = ec.CASES['sediment']
    xw, yw = plugins.RayleighEllipticity(per60).run_model(h, vp, np.array([0., 1.8, 3.2, 3.7, 4.4]), rho)
    assert np.isnan(xw) and np.isnan(yw)
    q = plugins.RayleighEllipticity(per60)
    q.set_modelparams(absolute=False)
    y = q.run_model(h, vp, vs, rho)[1]
    assert (y < 0).sum() > 3 and (y > 0).sum() > 3


def test_joint_target_values_the_ellipticity_with_the_host_likelihood(engines):
    from bayhunter_amd import plugins, targets
    per, (H, VP, VS, RHO, nl), res = engines
    b = int(np.nonzero(res['plain'][2][:, 0] == 0)[0][0])
    n = int(nl[b])
    h, vp, vs, rho = (a[b, :n] for a in (H, VP, VS, RHO))
    rng = np.random.RandomState(1)
    ydisp = plugins.SurfDisp(per, 'rdispph').run_model(h, vp, vs, rho)[1]
    yell = plugins.RayleighEllipticity(per).run_model(h, vp, vs, rho)[1]
    t1 = targets.RayleighDispersionPhase(per, ydisp + rng.normal(0, 0.02, 21))
    t2 = targets.RayleighEllipticity(per, yell + rng.normal(0, 0.03, 21), yerr=np.full(21, 0.03))
    joint = targets.JointTarget([t1, t2])
    joint.set_target_covariance([True, False], [0.0, 0.3])       # diagonal for the dispersion, exponential for H/V
    noise = np.array([0.0, 0.02, 0.3, 0.03])
    joint.evaluate(h, vp, vs, noise, rho=rho)
    want = 0.0
    for t, ymod, (corr, sigma) in ((t1, ydisp, noise[:2]), (t2, yell, noise[2:])):
        ydiff = ymod - t.obsdata.y
        c_inv, logdet = t.get_covariance(sigma=sigma, size=21, yerr=t.obsdata.yerr, corr=corr)
        want += t.valuation.get_likelihood(t.obsdata.y, ymod, c_inv, logdet)
    assert np.isfinite(want) and abs(joint.proposallikelihood - want) <= 1e-9 * abs(want)
    assert len(joint.proposalmisfits) == 3 and abs(joint.proposalmisfits[1] - np.sqrt(np.mean((yell - t2.obsdata.y) ** 2))) < 1e-12
