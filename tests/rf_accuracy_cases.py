"""Shared by test_rf_accuracy.py (CPU tier) and test_gpu_rf_accuracy.py (GPU tier): the forward part of rf_kernel --
flattening, interface coefficients, layer propagation, spectral division -- and the transform behind it, held to a
fraction of the REFERENCE'S OWN rounding error instead of the fixed TOL_RF.

Three traces per model, besides the one under test:

    O   the fp64 oracle (oracle.pyoracle: rf_model, or synrf for a model with its own Q)
    X   the same algorithm in long double (tests/hp_oracle.py: rf_model_ld / rf_model_q_ld), computed once per family
        and session
    R   the host replay of the device program with the device math (tests/rf_floor_cases.py: replay)

THE JUDGE, per family F and model b, with scale = max(1, max|O|) and T the trace under test (R on the CPU tier, the
device trace G on the GPU tier):

    e_ref(b) = max|O - X| / scale          how far the oracle itself is from the exact trace of the algorithm
    Y(b)     = max(e_ref(b), median over F of e_ref)        (the median shields a model on which the oracle was lucky)
    d(b)     = max|T - O| / scale
    assert   d(b) <= RF_TIGHT_MAX * Y(b) for every model, median over F of d / Y <= RF_TIGHT_MED,
             T finite exactly where O is finite

and on the GPU tier the same two bounds for |G - R| in place of |T - O|.  RF_TIGHT_MAX, RF_TIGHT_MED and the
measurements they were frozen from are in tests/tolerances.py.  Rows that are not finite in O take part in the
finiteness assertion only; a family must keep at least half its rows finite, except P_14, which exists for its NaN rows.

THE FAMILIES (every model of a family is judged; nout = nsamp everywhere: the whole trace):

    batch          B = 1, 2, 3, 4, 7 in five launches: one, two, three models of a workgroup, 3 + 1, 3 + 3 + 1
    L2 L10 L31     that many layers; L100: BH_MAX_LAYERS; ragged: 2 .. 15 layers in one batch
    n8 .. n4096    every transform length, eight models each, four at 2048 and 4096
    P_4to8, SV_4to8    incident P / SV at 4, 5, 6, 7, 8 s/deg
    SV_14          14 s/deg, post-critical for vp > 7.94 km/s: complex interface matrices
    P_14           the same models under incident P: the direct wave's delay is NaN, and so is the row, in O and in T
    a0.8 a1.0      Gauss factors with the 3e-19 cut-off active (rf_host.h); a1.21 a2.5: every frequency computed
    nsv            the rotation velocity given (3.1 km/s) instead of derived from the top layer
    lvz20_sv       twenty layers with velocity inversions (sorted_vs=False), incident SV, a = 2.5 (rows 0 .. 44), and in
                   the same family the three models of rf_extreme.ill_conditioned_models(), each a launch of its own
                   with its own constants (rows 45, 46, 47): SV on 20-odd layers with inversions as well, where the
                   oracle is 2.5e-9 ... 1e-7 from the exact trace and Y is the model's own e_ref
    sets_P sets_SV per-row slowness (bh_rf_batch_sets): two slownesses interleaved within a workgroup, each row judged
                   against the oracle at its own slowness
    lowq           rf_floor_cases.mixed_bound_models: Q_s = 5, Q_p = 10 -- the oracle's synrf entry takes Q per layer,
                   so does the long-double build of it, and so do the replay and bh_rf_batch
"""
import numpy as np

import hp_oracle
from bayhunter_amd import _lib as _abi
from bayhunter_amd.synthetic import draw_models
from rf_extreme import ill_conditioned_models
from rf_floor_cases import GAUSS_ALL, mixed_bound_models, replay

LENGTHS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
SLOWNESSES = [4.0, 5.0, 6.0, 7.0, 8.0]
MAX_FAMILY, MAX_LONG = 48, 4            # models per family; per family of 2048 samples and more
NAN_FAMILY = 'P_14'
N_LVZ = 45                              # drawn models of lvz20_sv; the three ill-conditioned ones follow
_CACHE = {}


def _launch(models, QP=None, QS=None, sets=None, **par):
    """One device call: models = (H, VP, VS, RHO, nl) as draw_models returns them; par overrides the defaults below;
    sets = (table of slownesses in s/deg, set index per row) for bh_rf_batch_sets."""
    d = dict(p=6.4, gauss=1.0, nsamp=512, fsamp=5.0, tshift=5.0, nsv=None, waveno=0)
    d.update(par)
    d['nout'] = d['nsamp']
    H, VP, VS, RHO, nl = models
    return dict(H=H, VP=VP, VS=VS, RHO=RHO, nl=np.asarray(nl, dtype=np.int32), QP=QP, QS=QS, sets=sets, par=d)


def _one(m, **par):
    """a single model given as a dict of its layers"""
    a = [np.ascontiguousarray(m[k], dtype=np.float64)[None, :] for k in ('h', 'vp', 'vs', 'rho')]
    return _launch((a[0], a[1], a[2], a[3], [a[0].shape[1]]), **par)


def _pack(models):
    """dicts of layers of different lengths -> zero-padded [B][Lmax] arrays, Q included"""
    B, L = len(models), max(m['h'].size for m in models)
    a = {k: np.zeros((B, L)) for k in ('h', 'vp', 'vs', 'rho')}
    q = {'qp': np.full((B, L), 500.0), 'qs': np.full((B, L), 225.0)}
    nl = np.zeros(B, dtype=np.int32)
    for b, m in enumerate(models):
        nl[b] = n = m['h'].size
        for k in a:
            a[k][b, :n] = m[k]
        for k in q:
            q[k][b, :n] = m[k]
    return (a['h'], a['vp'], a['vs'], a['rho'], nl), q['qp'], q['qs']


def _families():
    F = {}
    F['batch'] = [_launch(draw_models(B, (4, 10), seed=40 + B, Lmax=10)) for B in (1, 2, 3, 4, 7)]
    for L in (2, 10, 31):
        F['L%d' % L] = [_launch(draw_models(12, L, seed=50 + L))]
    F['L%d' % _abi.MAX_LAYERS] = [_launch(draw_models(4, _abi.MAX_LAYERS, seed=150, zmax=150.0))]
    F['ragged'] = [_launch(draw_models(24, (2, 15), seed=52, Lmax=15))]
    for n in LENGTHS:
        F['n%d' % n] = [_launch(draw_models(4 if n >= 2048 else 8, (3, 10), seed=60 + n, Lmax=10), nsamp=n, tshift=min(5.0, n / 25.0), gauss=2.0)]
    for tag, waveno in (('P', 0), ('SV', 1)):
        F['%s_4to8' % tag] = [_launch(draw_models(8, (4, 10), seed=100 + 10 * waveno + k, Lmax=10), p=p, waveno=waveno)
                              for k, p in enumerate(SLOWNESSES)]
    post = draw_models(7, 10, seed=90)
    assert 2 <= (post[1].max(axis=1) * 14.0 * 0.00899 > 1.0).sum() <= 5
    F['SV_14'] = [_launch(post, p=14.0, waveno=1)]
    F[NAN_FAMILY] = [_launch(post, p=14.0, waveno=0)]
    for a in (0.8, 1.0, 1.21, 2.5):
        F['a%g' % a] = [_launch(draw_models(12, (3, 10), seed=70, Lmax=10), gauss=a)]
    F['nsv'] = [_launch(draw_models(8, (3, 10), seed=71, Lmax=10), nsv=3.1)]
    F['lvz20_sv'] = [_launch(draw_models(N_LVZ, 20, seed=120, sorted_vs=False), waveno=1, gauss=2.5)]
    F['lvz20_sv'] += [_one(m, p=m['p'], gauss=m['gauss'], nsamp=m['nsamp'], fsamp=m['fsamp'], tshift=m['tshift'],
                           waveno=m['waveno']) for m in ill_conditioned_models()]
    # B = 7 with three models per workgroup: rows 0 1 2 | 3 4 5 | 6, the two slownesses alternate inside each
    F['sets_P'] = [_launch(draw_models(7, (4, 10), seed=130, Lmax=10), sets=([5.0, 7.5], [0, 1, 0, 1, 0, 1, 0]), p=123.0)]
    F['sets_SV'] = [_launch(draw_models(7, (4, 10), seed=131, Lmax=10), sets=([8.0, 4.5], [1, 0, 0, 1, 1, 0, 1]), p=123.0,
                            waveno=1)]
    models, QP, QS = _pack(list(mixed_bound_models(6)))      # (at one slowness, not each model's own draw: one launch)
    F['lowq'] = [_launch(models, QP=QP, QS=QS, gauss=GAUSS_ALL)]
    for name, launches in F.items():
        count = sum(len(l['nl']) for l in launches)
        assert count <= (MAX_LONG if max(l['par']['nsamp'] for l in launches) >= 2048 else MAX_FAMILY), name
    return F


FAMILIES = _families()
NAMES = list(FAMILIES)


def rows(launch):
    """[(h, vp, vs, rho, qp or None, qs or None, slowness of the row)] of a launch, each model cut to its layers"""
    out = []
    for b, n in enumerate(launch['nl']):
        q = [None if launch[k] is None else launch[k][b, :n] for k in ('QP', 'QS')]
        p = launch['par']['p'] if launch['sets'] is None else launch['sets'][0][launch['sets'][1][b]]
        out.append(tuple(launch[k][b, :n] for k in ('H', 'VP', 'VS', 'RHO')) + (q[0], q[1], float(p)))
    return out


def _oracle(launch, h, vp, vs, rho, qp, qs, p):
    from oracle import pyoracle
    par = launch['par']
    if qp is None:
        return pyoracle.rf_model(h, vp, vs, rho, p, par['gauss'], par['nsamp'], par['fsamp'], par['tshift'], par['nsv'],
                                 par['waveno'], par['nout'])
    z = np.concatenate(([0], np.cumsum(h)[:-1]))
    vpvs = float(vp[0]) / float(vs[0])
    return pyoracle.synrf(z, vp, vs, rho, qp, qs, p, par['gauss'], par['nsamp'], par['fsamp'], par['tshift'],
                          float(vs[0]) if par['nsv'] is None else par['nsv'], (2 - vpvs**2) / (2 - 2 * vpvs**2),
                          par['waveno'])[2][:par['nout']]


def _exact(launch, h, vp, vs, rho, qp, qs, p):
    par = launch['par']
    tail = (p, par['gauss'], par['nsamp'], par['fsamp'], par['tshift'], par['nsv'], par['waveno'], par['nout'])
    return hp_oracle.rf_model_ld(h, vp, vs, rho, *tail) if qp is None else hp_oracle.rf_model_q_ld(h, vp, vs, rho, qp, qs, *tail)


def reference(name):
    """The family's yardstick, computed once per session: O and X per model, the rows O leaves finite, scale, e_ref
    and Y (NaN on a row that is not finite in O)."""
    if name in _CACHE:
        return _CACHE[name]
    O, X = [], []
    for launch in FAMILIES[name]:
        for r in rows(launch):
            O.append(_oracle(launch, *r))
            X.append(_exact(launch, *r))
    B = len(O)
    ok = np.array([bool(np.isfinite(o).all()) for o in O])
    scale, e_ref = np.full(B, np.nan), np.full(B, np.nan)
    for b in np.flatnonzero(ok):
        scale[b] = max(1.0, np.abs(O[b]).max())
        e_ref[b] = float(np.abs(O[b].astype(np.longdouble) - X[b]).max()) / scale[b]
    Y = np.maximum(e_ref, np.median(e_ref[ok])) if ok.any() else e_ref
    _CACHE[name] = dict(O=O, X=X, ok=ok, scale=scale, e_ref=e_ref, Y=Y)
    return _CACHE[name]


def host_replay(name):
    """R of every model of the family, computed once per session"""
    if ('R', name) not in _CACHE:
        R = []
        for launch in FAMILIES[name]:
            par = launch['par']
            for h, vp, vs, rho, qp, qs, p in rows(launch):
                R.append(replay(h, vp, vs, rho, p, par['gauss'], par['nsamp'], par['fsamp'], par['tshift'], par['nsv'],
                                par['waveno'], par['nout'], qp=qp, qs=qs))
        _CACHE[('R', name)] = R
    return _CACHE[('R', name)]


def well_posed(name):
    """None, or what is wrong with the family as a test: the extended-precision trace finite where the oracle is, an
    error of the oracle that can be measured, and enough finite rows."""
    c = reference(name)
    for b, (o, x) in enumerate(zip(c['O'], c['X'])):
        if not np.array_equal(np.isfinite(o), np.isfinite(x.astype(np.float64))):
            return 'row %d: the oracle and its long-double build are not finite in the same samples' % b
        if np.isfinite(o).any() and not np.isfinite(o).all():
            return 'row %d: the oracle\'s trace is finite in part' % b
    if not c['ok'].any() or not (c['e_ref'][c['ok']] > 0).all():
        return 'no finite row, or an oracle error of zero'
    if name != NAN_FAMILY and 2 * c['ok'].sum() < c['ok'].size:
        return 'fewer than half of the rows are finite'
    if name == NAN_FAMILY and c['ok'].all():
        return 'no NaN row'
    return None


def judge(name, T, c_max, c_med, against=None, tag=''):
    """(worst d / Y, median d / Y, None or the first failure).  T: the traces under test, one per model in the order of
    rows(); against: the traces to measure the distance from (default the oracle's; the scale and Y stay the oracle's).
    Prints the family's line."""
    c = reference(name)
    ref = c['O'] if against is None else against
    assert len(T) == len(ref) == c['ok'].size
    msg = None
    ratio = np.full(c['ok'].size, np.nan)
    for b in range(c['ok'].size):
        t = np.asarray(T[b], dtype=np.float64)
        if t.shape != c['O'][b].shape or not np.array_equal(np.isfinite(t), np.isfinite(c['O'][b])):
            msg = msg or 'row %d is not finite exactly where the oracle is' % b
        elif c['ok'][b]:
            ratio[b] = float(np.abs(t - ref[b]).max()) / c['scale'][b] / c['Y'][b]
    ok = c['ok'] & np.isfinite(ratio)
    worst = float(ratio[ok].max()) if ok.any() else float('nan')
    med = float(np.median(ratio[ok])) if ok.any() else float('nan')
    print('RF-RATIO %s %-8s rows=%d/%d e_ref median %.2e max %.2e | d/Y worst %.4f (row %d) median %.5f'
          % (tag, name, ok.sum(), ok.size, np.median(c['e_ref'][c['ok']]), c['e_ref'][c['ok']].max(), worst,
             int(np.nanargmax(ratio)) if ok.any() else -1, med))
    if msg is None and not ok.any():
        msg = 'no finite row'
    if msg is None and not worst <= c_max:
        msg = 'row %d: d / Y = %.4f above %.3g' % (int(np.nanargmax(ratio)), worst, c_max)
    if msg is None and not med <= c_med:
        msg = 'family median of d / Y = %.5f above %.3g' % (med, c_med)
    return worst, med, msg
