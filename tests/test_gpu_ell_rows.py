"""ell_rows_kernel (bh_ell_batch_rows) against ell_kernel (bh_ell_batch) on the same device inputs.

* Values: bit for bit bh_ell_batch's, NaNs at the same positions, nothing written behind a row's nper values -- at 1, 4,
  13 and 130 ragged models of 2-16 layers and 1, 21, 43 and 60 periods (256, 12, 5 and 4 models per workgroup: partial
  last workgroups, idle threads at 43 periods, models crossing wave boundaries), without an order, with the identity
  and with a random permutation; flat earth, and one flattened-earth case.
* Flags: with raise_flag the word of a model whose flag was 0 and whose row holds a NaN becomes BH_ELL_NO_VALUE; every
  other word of err -- set flags, good rows, the neighbouring columns -- is unchanged; without raise_flag err is only read.
* Arguments are refused before any device work (this test needs no device).
"""
import ctypes as C

import numpy as np
import pytest

import ellipticity_cases as ec

gpu = pytest.mark.gpu

BMAX, LMAX = 130, 16
PER = np.linspace(1., 41., 60)
NO_VALUE = 4                       # BH_ELL_NO_VALUE


def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(device='cuda', dtype=dtype)


@pytest.fixture(scope='module')
def batch(lib):
    """130 ragged models (2-16 layers, [B, 16]) and the phase velocities bh_swd_batch finds for them at PER on the flat
    and on the flattened earth: the input both kernels share.  Behind its last layer a model holds garbage, which
    neither kernel reads."""
    import torch
    from bayhunter_amd import _lib
    rng = np.random.RandomState(7)
    nlay = rng.randint(2, LMAX + 1, BMAX).astype(np.int32)
    nlay[:4] = (2, LMAX, 3, 10)
    Z = np.zeros((4, BMAX, LMAX))
    for b in range(BMAX):
        n = nlay[b]
        for i, x in enumerate(ec.stack(n, 100 + b, lvz=(b % 3 == 0 and n > 4))):
            Z[i, b, :n] = np.asarray(x, dtype=np.float64).astype(np.float32)
    d = [_dev(Z[i], torch.float64) for i in range(4)]
    tg = (_lib.SwdTarget * 2)(_lib.SwdTarget(2, 0, 1, 0, 60, 0, 0, 0), _lib.SwdTarget(2, 0, 1, 1, 60, 0, 60, 0))
    out = torch.zeros((BMAX, 120), dtype=torch.float64, device='cuda')
    err = torch.zeros((BMAX, 2), dtype=torch.int32, device='cuda')
    dn, dper = _dev(nlay, torch.int32), _dev(PER, torch.float64)
    _lib.check(lib.bh_swd_batch(BMAX, LMAX, LMAX, dn.data_ptr(), *[x.data_ptr() for x in d], 2, tg, dper.data_ptr(),
                                out.data_ptr(), 120, err.data_ptr(), None, 0, None))
    torch.cuda.synchronize()
    out, err = out.cpu().numpy(), err.cpu().numpy()
    assert not err.any() and np.all(out > 0)
    M = rng.choice([np.nan, 1e30, -1.0, 0.0, 7.7], size=Z.shape)
    for b in range(BMAX):
        M[:, b, :nlay[b]] = Z[:, b, :nlay[b]]
    return M, nlay, out[:, :60].copy(), out[:, 60:].copy()


def _case(batch, B, nper, flsph=0):
    """The inputs of one comparison: rows without an ellipticity among good ones, err with the source's flags in its
    middle column of three."""
    M, nlay, C0, C1 = batch
    M, nlay = M[:, :B].copy(), nlay[:B].copy()
    c = np.full((B, nper + 3), 123.0)                       # strides wider than nper; the padding is never read
    c[:, :nper] = (C1 if flsph else C0)[:B, :nper]
    err = np.zeros((B, 3), dtype=np.int32)
    err[:, 0], err[:, 2] = 7, 9                             # other targets' flags
    c[0, 0] = np.nan
    expect = {0}                                            # rows that must be flagged
    if B >= 4:
        M[2, 1, 0] = 0.0                                    # water on top
        nlay[2] = 1                                         # a half-space alone
        expect |= {1, 2}
    if B >= 13:
        err[5, 1], err[7, 1] = 1, 2                         # set flags: NaN rows, the words stay
        nlay[6] = LMAX + 1                                  # not a model of this batch's depth
        c[8, nper - 1], c[9, 0] = 0.0, np.inf
        expect |= {6, 8, 9}
    return M, nlay, c, err, expect


def _run(lib, fn, M, nlay, per, flsph, c, err, absolute, order=None, raise_flag=None):
    import torch
    from bayhunter_amd import _lib
    B, nper = nlay.size, per.size
    d = [_dev(M[i], torch.float64) for i in range(4)]
    dn, dper, dc, de = _dev(nlay, torch.int32), _dev(per, torch.float64), _dev(c, torch.float64), _dev(err, torch.int32)
    out = torch.full((B, nper + 3), -777.0, dtype=torch.float64, device='cuda')
    args = [B, LMAX, M.shape[2], dn.data_ptr(), *[x.data_ptr() for x in d], nper, dper.data_ptr(), flsph, dc.data_ptr(),
            c.shape[1], de.data_ptr() + 4, 3, 1 if absolute else 0, out.data_ptr(), nper + 3]
    if fn == 'rows':
        do = None if order is None else _dev(order, torch.int32)
        _lib.check(lib.bh_ell_batch_rows(*(args + [None if do is None else do.data_ptr(), raise_flag, None])))
    else:
        _lib.check(lib.bh_ell_batch(*(args + [None])))
    torch.cuda.synchronize()
    return out.cpu().numpy(), de.cpu().numpy()


def _order(kind, B):
    if kind == 'none':
        return None
    if kind == 'identity':
        return np.arange(B, dtype=np.int32)
    return np.random.RandomState(11 + B).permutation(B).astype(np.int32)


def _same_bits(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def _compare(lib, batch, B, nper, order, flsph=0):
    M, nlay, c, err, expect = _case(batch, B, nper, flsph)
    per = PER[:nper]
    absolute = nper != 21
    want, err_ref = _run(lib, 'dense', M, nlay, per, flsph, c, err, absolute)
    assert np.array_equal(err_ref, err)
    assert np.all(want[:, nper:] == -777.0)
    nan_row = np.isnan(want[:, :nper]).any(axis=1)
    assert set(np.nonzero(nan_row & (err[:, 1] == 0))[0]) == expect     # the rows the case made, no others
    if B >= 13:
        assert np.isnan(want[[5, 7], :nper]).all() and np.isfinite(want[[3, 4, 10, 11, 12], :nper]).all()
    # read-only: the values, and err as it was
    got, e0 = _run(lib, 'rows', M, nlay, per, flsph, c, err, absolute, _order(order, B), 0)
    assert _same_bits(got[:, :nper], want[:, :nper]) and np.all(got[:, nper:] == -777.0)
    assert np.array_equal(e0, err)
    # with the flag: the same values, BH_ELL_NO_VALUE exactly where the flag was 0 and the row holds a NaN
    got, e1 = _run(lib, 'rows', M, nlay, per, flsph, c, err, absolute, _order(order, B), 1)
    assert _same_bits(got[:, :nper], want[:, :nper]) and np.all(got[:, nper:] == -777.0)
    want_err = err.copy()
    want_err[sorted(expect), 1] = NO_VALUE
    assert np.array_equal(e1, want_err), np.nonzero(e1 != want_err)


@gpu
@pytest.mark.parametrize('order', ['none', 'identity', 'random'])
@pytest.mark.parametrize('nper', [1, 21, 43, 60])
@pytest.mark.parametrize('B', [1, 4, 13, 130])
def test_rows_are_the_dense_kernels_bit_for_bit_and_flags_go_where_they_belong(lib, batch, B, nper, order):
    _compare(lib, batch, B, nper, order)


@gpu
def test_flattened_earth(lib, batch):
    _compare(lib, batch, 65, 21, 'random', flsph=1)


def test_c_abi_refuses_bad_arguments_before_it_touches_a_device(lib):
    from bayhunter_amd import _lib
    p = C.c_void_p(64)            # never dereferenced: every call below is refused first

    def rows(nper=21, c_stride=21, err_stride=1, out_stride=21, null=None, Lmax=10, mstride=10, B=4):
        a = [B, Lmax, mstride, p, p, p, p, p, nper, p, 0, p, c_stride, p, err_stride, 1, p, out_stride, None, 1, None]
        if null is not None:
            a[null] = None
        return lib.bh_ell_batch_rows(*a)
    for kw in (dict(nper=0), dict(nper=_lib.MAX_PERIODS + 1), dict(c_stride=20), dict(out_stride=20), dict(err_stride=0),
               dict(Lmax=0), dict(Lmax=_lib.MAX_LAYERS + 1), dict(mstride=9), dict(B=-1)) + tuple(
                   dict(null=i) for i in (3, 4, 5, 6, 7, 9, 11, 13, 16)):
        assert rows(**kw) == _lib.BH_ERR_ARG, kw
        assert lib.bh_last_error()
    assert rows(B=0) == _lib.BH_OK                           # nothing to do: no device needed
