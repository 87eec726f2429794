"""The argument checks the three sensitivity batch entry points share (bh_sens_batch, bh_sens_group_batch,
bh_ell_sens_batch; csrc/sens_capi_common.h): one table of bad arguments against all three, each row with its return code
and the text bh_last_error then holds.  Every row is refused before the device is touched, so no GPU is needed and no
pointer is dereferenced."""
import pytest

P = 64                   # a pointer that is never dereferenced
COMMON = ['B', 'Lmax', 'mstride', 'nlay', 'h', 'vp', 'vs', 'rho']
TAIL = ['c', 'c_stride', 'c_err', 'err_stride', 'K']
# argument order, the doubles of workspace per (model, period), and the pointers that may be NULL
PASSES = {
    'sens': (COMMON + ['iwave', 'nper', 'periods', 'flsph'] + TAIL + ['c_out', 'dc_dT', 'ws', 'ws_bytes', 'stream'], 1, ()),
    'sens_group': (COMMON + ['iwave', 'nper', 'periods', 'flsph'] + TAIL
                   + ['U', 'dU_dT', 'c_out', 'K_phase', 'ws', 'ws_bytes', 'stream'], 6, ('K_phase',)),
    'ell_sens': (COMMON + ['nper', 'periods', 'flsph', 'absolute'] + TAIL
                 + ['E', 'dE_dT', 'c_out', 'K_phase', 'ws', 'ws_bytes', 'stream'], 3, ('K_phase',)),
}
INTS = dict(B=4, Lmax=8, mstride=8, iwave=2, nper=5, flsph=0, absolute=1, c_stride=5, err_stride=1, ws_bytes=1 << 20)

ARG, WORKSPACE = 'BH_ERR_ARG', 'BH_ERR_WORKSPACE'
TABLE = [
    (dict(B=-1), ARG, 'B/Lmax out of range'),
    (dict(Lmax=0), ARG, 'B/Lmax out of range'),
    (dict(Lmax=101, mstride=101), ARG, 'B/Lmax out of range'),
    (dict(mstride=7), ARG, 'model_stride < Lmax'),
    (dict(iwave=0), ARG, 'iwave is neither 1 (Love) nor 2 (Rayleigh)'),
    (dict(iwave=3), ARG, 'iwave is neither 1 (Love) nor 2 (Rayleigh)'),
    (dict(nper=0), ARG, 'nper out of range (1 .. 60)'),
    (dict(nper=61, c_stride=61), ARG, 'nper out of range (1 .. 60)'),
    (dict(flsph=1), ARG, 'flsph: sensitivity kernels are formed on a flat earth only'),
    (dict(c_stride=4), ARG, 'c_stride shorter than nper'),
    (dict(err_stride=0), ARG, 'err_stride < 1'),
    (dict(ws_bytes='short'), WORKSPACE, 'workspace too small (bh_%s_workspace_bytes)'),
    (dict(ws=None), WORKSPACE, 'workspace too small (bh_%s_workspace_bytes)'),
    # 2^31 - 1 models of 100 layers at 60 periods are more than 2^31 - 1 workgroups
    (dict(B=0x7fffffff, Lmax=100, mstride=100, nper=60, c_stride=60, ws_bytes=1 << 62), ARG,
     'B * nper * 4 * Lmax lanes do not fit one launch'),
]


def _call(lib, name, **kw):
    order, wsn, _ = PASSES[name]
    if kw.get('ws_bytes') == 'short':
        kw['ws_bytes'] = INTS['B'] * INTS['nper'] * wsn * 8 - 1
    args = [kw[a] if a in kw else INTS.get(a, None if a == 'stream' else P) for a in order]
    return getattr(lib, 'bh_%s_batch' % name)(*args)


@pytest.mark.parametrize('name', sorted(PASSES))
def test_batch_entry_point_refuses_the_table(lib, name):
    from bayhunter_amd import _lib
    order, wsn, optional = PASSES[name]
    rows = [r for r in TABLE if set(r[0]) <= set(order)]          # a pass without an iwave skips those rows
    assert len(rows) == len(TABLE) - (0 if 'iwave' in order else 2)
    required = [a for a in order if a not in INTS and a not in optional + ('ws', 'stream')]
    assert len(required) == (11 if name == 'sens' else 12)
    rows += [({a: None}, ARG, 'NULL pointer') for a in required]
    for kw, code, text in rows:
        assert _call(lib, name, **kw) == getattr(_lib, code), kw
        assert lib.bh_last_error().decode() == (text % name if '%s' in text else text), kw
    # an optional pointer may be NULL: the call then gets as far as the workspace check
    for a in optional:
        assert _call(lib, name, ws_bytes='short', **{a: None}) == _lib.BH_ERR_WORKSPACE
    # the checks come in this order: the first bad argument decides
    assert _call(lib, name, B=-1, flsph=1, ws=None) == _lib.BH_ERR_ARG and lib.bh_last_error() == b'B/Lmax out of range'
    assert _call(lib, name, flsph=1, K=None, ws=None) == _lib.BH_ERR_ARG and lib.bh_last_error().startswith(b'flsph')
    assert _call(lib, name, K=None, ws=None) == _lib.BH_ERR_ARG and lib.bh_last_error() == b'NULL pointer'
    # an empty batch is done before the workspace is looked at
    assert _call(lib, name, B=0, ws=None, ws_bytes=0) == _lib.BH_OK
    assert getattr(lib, 'bh_%s_workspace_bytes' % name)(4, 5) == 4 * 5 * wsn * 8
    assert getattr(lib, 'bh_%s_workspace_bytes' % name)(-1, 5) == 0 == getattr(lib, 'bh_%s_workspace_bytes' % name)(4, -1)
