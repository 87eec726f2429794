"""rf_kernel with the wave-uniform choice of the attenuation exponent's form and the radix-4 passes of its inverse
transform, on the GPU against the host replay of rf_host.h (tests/rf_floor_cases.py), to the tolerance the RF GPU tests
use (TOL_RF relative to the trace's scale): partial workgroups and task rounds, every transform length class, the
Gauss cut-off on and off, waves that take the full form next to waves that take the short one, the per-row form,
complex interface coefficients, and a NaN model among good ones."""
import numpy as np
import pytest

from bayhunter_amd.synthetic import draw_models
from rf_floor_cases import GAUSS_ALL, mixed_bound_models, replay
from tolerances import TOL_RF

pytestmark = pytest.mark.gpu


def _gpu(lib, H, VP, VS, RHO, nl, QP=None, QS=None, p=6.4, gauss=1.0, nsamp=512, fsamp=5.0, tshift=5.0, waveno=0,
         nout=201, sets=None):
    """bh_rf_batch, or bh_rf_batch_sets with sets = (table, set_id)"""
    import torch
    from bayhunter_amd import _lib
    dev = torch.device('cuda')
    B, L = H.shape

    def up(a, dt=np.float64):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = [up(a) for a in (H, VP, VS, RHO, QP, QS)]
    ptr = [None if x is None else x.data_ptr() for x in d]
    dn = up(nl, np.int32)
    out = torch.full((B, nout), 7.0, dtype=torch.float64, device=dev)
    par = _lib.RfParams(p, gauss, fsamp, tshift, -1.0, nsamp, waveno, nout, 0)
    if sets is None:
        _lib.check(lib.bh_rf_batch(B, L, L, dn.data_ptr(), *ptr, par, out.data_ptr(), nout, None, 0, None))
    else:
        t, i = up(sets[0]), up(sets[1], np.int32)
        _lib.check(lib.bh_rf_batch_sets(B, L, L, dn.data_ptr(), *ptr, par, len(sets[0]), t.data_ptr(), i.data_ptr(),
                                        out.data_ptr(), nout, None, 0, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _host(H, VP, VS, RHO, nl, QP=None, QS=None, **kw):
    return np.stack([replay(H[b, :nl[b]], VP[b, :nl[b]], VS[b, :nl[b]], RHO[b, :nl[b]],
                            qp=None if QP is None else QP[b, :nl[b]], qs=None if QS is None else QS[b, :nl[b]], **kw)
                     for b in range(H.shape[0])])


def _close(got, want, tag):
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), tag
    ok = np.isfinite(want).all(axis=1)
    scale = np.maximum(1.0, np.abs(want[ok]).max(axis=1))
    worst = float((np.abs(got[ok] - want[ok]).max(axis=1) / scale).max()) if ok.any() else 0.0
    print('gpu rf_floor, %s: worst %.3e over %d finite of %d rows' % (tag, worst, ok.sum(), ok.size))
    assert worst <= TOL_RF, (tag, worst)
    return int(ok.sum())


def _pack(models, L):
    B = len(models)
    a = {k: np.zeros((B, L)) for k in ('h', 'vp', 'vs', 'rho')}
    q = {'qp': np.full((B, L), 500.0), 'qs': np.full((B, L), 225.0)}
    nl = np.zeros(B, dtype=np.int32)
    for b, m in enumerate(models):
        n = m['h'].size
        nl[b] = n
        for k in a:
            a[k][b, :n] = m[k]
        for k in q:
            q[k][b, :n] = m[k]
    return a['h'], a['vp'], a['vs'], a['rho'], nl, q['qp'], q['qs']


def _plain(H, VP, VS, RHO, nl, b):
    n = nl[b]
    return dict(h=H[b, :n], vp=VP[b, :n], vs=VS[b, :n], rho=RHO[b, :n], qp=np.full(n, 500.0), qs=np.full(n, 225.0))


@pytest.mark.parametrize('B', [1, 2, 3, 4, 7])
def test_partial_workgroups_and_task_rounds(lib, B):
    """Three models per workgroup: one, two (partial), three, 3 + 1, 3 + 3 + 1; 213 tasks per model in rounds of 256."""
    m = draw_models(B, (4, 10), seed=40 + B, Lmax=10)
    assert _close(_gpu(lib, *m), _host(*m), 'B = %d' % B) == B


@pytest.mark.parametrize('L', [2, 10, 15])
def test_layer_counts(lib, L):
    m = draw_models(4, L, seed=50 + L)
    assert _close(_gpu(lib, *m), _host(*m), 'L = %d' % L) == 4


@pytest.mark.parametrize('nsamp', [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096])
def test_transform_lengths(lib, nsamp):
    """log2 n odd (128, 512: a radix-2 stage, then radix-4 passes) and even (256, 1024: radix-4 passes only)"""
    m = draw_models(4, (3, 10), seed=60 + nsamp, Lmax=10)
    kw = dict(nsamp=nsamp, nout=min(201, nsamp), tshift=min(5.0, nsamp / 25.0), gauss=2.0)
    assert _close(_gpu(lib, *m, **kw), _host(*m, **kw), 'nsamp = %d' % nsamp) == 4


@pytest.mark.parametrize('gauss,nact', [(0.8, 171), (1.0, 213), (1.21, 257)])
def test_gauss_cut_off(lib, gauss, nact):
    """a = 0.8 and 1.0: frequencies behind the 3e-19 cut-off are zero-filled; a = 1.21: all 257 are computed."""
    from bayhunter_amd import _lib
    par = _lib.RfParams(6.4, gauss, 5.0, 5.0, -1.0, 512, 0, 201, 0)
    assert int(lib.bh_rf_active_frequencies(par)) == nact
    m = draw_models(4, (3, 10), seed=70, Lmax=10)
    assert _close(_gpu(lib, *m, gauss=gauss), _host(*m, gauss=gauss), 'a = %g' % gauss) == 4


@pytest.fixture(scope='module')
def mixed():
    """One workgroup of three models, 257 tasks each, model-major: a Q_s = 5 model (its first wave holds arguments on
    both sides of the bound, its other waves only outside: the full form) between or before crustal-Q models (inside: the
    short form); the wave with tasks 256 .. 319 holds the last frequency of one model and the first 63 of the next."""
    lo = list(mixed_bound_models(2))
    H, VP, VS, RHO, nl = draw_models(4, (4, 6), seed=80, Lmax=6)
    hi = [_plain(H, VP, VS, RHO, nl, b) for b in range(4)]
    groups = [[lo[0], hi[0], hi[1]], [hi[2], lo[1], hi[3]], [lo[0], lo[1], hi[0]]]
    return [_pack(g, 6) for g in groups]


def test_full_and_short_form_in_neighbouring_waves(lib, mixed):
    for k, g in enumerate(mixed):
        H, VP, VS, RHO, nl, QP, QS = g
        kw = dict(gauss=GAUSS_ALL, nout=512)
        got = _gpu(lib, H, VP, VS, RHO, nl, QP, QS, **kw)
        assert _close(got, _host(H, VP, VS, RHO, nl, QP, QS, **kw), 'mixed group %d' % k) == 3
        # a model's trace does not depend on which models share its waves: alone in its workgroup, the same bits
        for b in range(3):
            alone = _gpu(lib, *[a[b:b + 1] for a in g], **kw)
            assert np.array_equal(alone[0], got[b]), (k, b)


def test_uniform_and_per_row_form_agree_bit_for_bit(lib, mixed):
    for g in mixed:
        H, VP, VS, RHO, nl, QP, QS = g
        for p in (6.4, 14.0):
            kw = dict(gauss=GAUSS_ALL, waveno=1)
            uni = _gpu(lib, H, VP, VS, RHO, nl, QP, QS, p=p, **kw)
            row = _gpu(lib, H, VP, VS, RHO, nl, QP, QS, p=123.0, sets=([5.0, p], [1, 1, 1]), **kw)
            assert np.isfinite(uni).all() and np.array_equal(uni, row), p


@pytest.mark.parametrize('waveno', [0, 1])
def test_complex_coefficients_at_14_s_per_deg(lib, waveno):
    """0.126 s/km is post-critical for vp > 7.94 km/s: complex interface matrices.  Incident P (waveno 0): the direct
    wave's delay is NaN and so is the row, on the device as in the replay; incident SV: finite."""
    H, VP, VS, RHO, nl = draw_models(7, 10, seed=90)
    post = VP.max(axis=1) * 14.0 * 0.00899 > 1.0
    assert 2 <= post.sum()
    got = _gpu(lib, H, VP, VS, RHO, nl, p=14.0, waveno=waveno)
    nfin = _close(got, _host(H, VP, VS, RHO, nl, p=14.0, waveno=waveno), '14 s/deg, waveno %d' % waveno)
    assert nfin == (7 if waveno else 7 - post.sum())


def test_nan_model_among_good_ones(lib):
    H, VP, VS, RHO, nl = draw_models(7, (4, 10), seed=91, Lmax=10)
    good = _gpu(lib, H, VP, VS, RHO, nl)
    VSn = VS.copy()
    VSn[4, 1] = np.nan
    got = _gpu(lib, H, VP, VSn, RHO, nl)
    assert np.isnan(got[4]).all() and np.isfinite(good).all()
    keep = np.arange(7) != 4
    assert np.array_equal(got[keep], good[keep])
