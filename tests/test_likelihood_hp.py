"""The extended-precision likelihood reference (tests/likelihood_hp.py) and its bounds, proven on the CPU before
they judge a kernel (tests/test_gpu_likelihood_hp.py):

* the restatement reproduces the reference's own golden vectors and the host mirror's closed forms;
* a plain fp64 numpy evaluation (einsum / dot) of EVERY case of the shared table stays inside the derived
  bounds -- the bounds are not too tight for a correct fp64 implementation;
* a dropped column of a 201-point target with residuals of 1e-3 is far outside them -- they are not vacuous."""
import os

import numpy as np
import pytest

import likelihood_hp as hp
from conftest import GOLDEN
from test_likelihood import CASES as GOLDEN_CASES, RTOL, _targets


def _descriptors(joint):
    """Target descriptors and aux of a two-target JointTarget whose rows are [target 0 | target 1]."""
    aux, targets, off = [], [], 0
    for t in joint.targets:
        n, a, extra = t.obsdata.y.size, None, 0.0
        if t.covmodel == hp.COV_NOCORR_SCALED:
            a = t.obsdata.yerr / t.obsdata.yerr.min()
            extra = float(np.log(np.prod(a)))
        elif t.covmodel == hp.COV_GAUSS:
            a, extra = t.valuation.corr_inv.ravel(), float(t.valuation.logcorr_det)
        targets.append(hp.Target(n, off, t.covmodel, sum(x.size for x in aux), extra))
        if a is not None:
            aux.append(np.asarray(a, dtype=np.float64))
        off += n
    return targets, np.concatenate(aux + [np.zeros(1)])


@pytest.mark.parametrize('case', sorted(GOLDEN_CASES))
def test_restatement_reproduces_the_golden_likelihoods(case):
    g = np.load(os.path.join(GOLDEN, 'likelihood.npz'))
    with_yerr, setup = GOLDEN_CASES[case]
    T, t1, t2 = _targets(g, with_yerr)
    joint = T.JointTarget([t1, t2])
    joint.set_target_covariance([s[0] for s in setup], [s[1] for s in setup], rcond=1e-5)
    targets, aux = _descriptors(joint)
    out = np.concatenate([np.nan_to_num(g['ysw']), g['yrf']], axis=1)
    yobs = np.concatenate([g['sw_y'], g['rf_y']])
    logL, mis, bl, bm = hp.evaluate(out, yobs, g[case + '_noise'], aux, targets, err=g['esw'].reshape(-1, 1))
    assert np.allclose(logL.astype(float), g[case + '_logL'], rtol=RTOL, atol=0)
    assert np.allclose(mis.astype(float), g[case + '_misfits'], rtol=RTOL, atol=0)
    assert logL[5] == -1e15 and np.all(mis[5] == 1e15) and bl[5] == 0 and np.all(bm[5] == 0)


@pytest.mark.parametrize('n', [1, 2, 3, 37, 201])
def test_restatement_reproduces_the_host_mirror(n):
    """targets.quadratic_form for all four forms, and d^T get_corr_inv d of the reference's matrix route."""
    from bayhunter_amd import targets as T
    rs = np.random.RandomState(n)
    d = rs.normal(size=n)
    yerr = rs.uniform(0.5, 2.0, size=n)
    t = T.RayleighDispersionPhase(np.linspace(0, 10, n), np.zeros(n), yerr=yerr)
    t.valuation.init_covariance_gauss(0.9, n, rcond=1e-6)
    se = yerr / yerr.min()
    for cov, corr, sigma in ((0, 0.0, 0.3), (1, 0.0, 0.3), (2, 0.7, 0.3), (2, -0.97, 0.02), (3, 0.9, 1.7)):
        t.covmodel = cov
        q, ld = t.quadratic_form(d, corr, sigma)
        want = -0.5 * (n * np.log(2 * np.pi) + ld) - q / 2.
        aux = se if cov == 1 else t.valuation.corr_inv.ravel()
        extra = float(np.log(np.prod(se))) if cov == 1 else float(t.valuation.logcorr_det) if cov == 3 else 0.0
        logL, mis, bl, bm = hp.evaluate(d[None, :], np.zeros(n), np.array([[corr, sigma]]), aux,
                                        [hp.Target(n, 0, cov, 0, extra)])
        assert np.isclose(float(logL[0]), want, rtol=1e-12, atol=0), (cov, n)
        assert np.isclose(float(mis[0, 0]), t.valuation.get_rms(np.zeros(n), d), rtol=1e-14)
        assert mis[0, 1] == mis[0, 0]
        if cov == 2:
            c_inv, logdet = t.valuation.get_covariance_exp(corr, sigma, n)
            assert np.isclose(float(logL[0]), -0.5 * (n * np.log(2 * np.pi) + logdet) - d.dot(c_inv).dot(d) / 2., rtol=1e-12)


def plain_fp64(k, rows):
    """The same inputs in plain fp64 numpy: einsum / dot, numpy's own summation orders."""
    c = k['case']
    out, yobs, noise, aux = k['out'], k['yobs'], k['noise'], k['aux']
    sets = np.zeros(len(rows), dtype=np.int64) if k['obs_id'] is None else k['obs_id'][rows].astype(np.int64)
    bad = (sets < 0) | (sets >= k['nsets'])
    if k['err'] is not None:
        bad |= k['err'][rows].any(axis=1)
    sets = np.where(bad, 0, sets)
    logL, mis = np.zeros(len(rows)), np.zeros((len(rows), k['T'] + 1))
    with np.errstate(all='ignore'):
        for t, tg in enumerate(k['targets']):
            n, sl = tg.n, slice(tg.off, tg.off + tg.n)
            d = out[rows, sl] - yobs[sets, sl]
            corr, sigma = noise[rows, 2 * t], noise[rows, 2 * t + 1]
            logdet = (2 * n) * np.log(sigma)
            if tg.cov == 0:
                madist = np.einsum('bi,bi->b', d, d) / sigma ** 2
                logdet = logdet + tg.logdet_extra
            elif tg.cov == 1:
                se = k['set_scale'][sets, sl] if c['tables'] else aux[tg.aux_off:tg.aux_off + n][None, :]
                madist = np.sum(d ** 2 / se, axis=1) / sigma ** 2
                logdet = logdet + (k['set_logdet'][sets, t] if c['tables'] else tg.logdet_extra)
            elif tg.cov == 2:
                w = np.repeat((1.0 + corr ** 2)[:, None], n, axis=1)
                w[:, 0] = w[:, -1] = 1.0
                q = np.einsum('bi,bi->b', w * d, d) - 2.0 * corr * np.einsum('bi,bi->b', d[:, :-1], d[:, 1:])
                madist = q / (sigma ** 2 * (1 - corr ** 2))
                logdet = logdet + (n - 1) * np.log(1 - corr ** 2)
            else:
                Rinv = aux[tg.aux_off:tg.aux_off + n * n].reshape(n, n)
                madist = np.einsum('bi,bi->b', d.dot(Rinv), d) / sigma ** 2
                logdet = logdet + tg.logdet_extra
            logL += -0.5 * (n * np.log(2 * np.pi) + logdet) - madist / 2.
            mis[:, t] = np.sqrt(np.mean(d ** 2, axis=1))
        mis[:, -1] = mis[:, :-1].sum(axis=1)
    logL[bad], mis[bad] = -1e15, 1e15
    return logL, mis


def _scatter(k, logL, mis):
    full_l, full_m = np.full(k['B'], np.nan), np.full((k['B'], k['T'] + 1), np.nan)
    full_l[k['rows']], full_m[k['rows']] = logL, mis
    return full_l, full_m


def test_case_table_covers_what_it_promises():
    by = {c['name']: c for c in hp.CASES}
    for cov in (0, 1, 2):
        assert {c['ns'][0] for c in hp.CASES if c['name'].startswith('len_') and c['forms'] == (cov,)} == set(hp.CLOSED_N)
    assert {c['ns'][0] for c in hp.CASES if c['name'].startswith('dense_pinv0.98')} == set(hp.DENSE_N)
    assert {c['B'] for c in hp.CASES if c['name'].startswith('batch_')} == set(hp.BATCHES)
    assert hp.SWITCH == 32768 and hp.LIKE_NMAX == 1024 and hp.LIKE_M == 8 and max(hp.CLOSED_N) == hp.LIKE_NMAX
    fused = {c['ns'][0] for c in hp.CASES if c['B'] > hp.SWITCH and c['forms'] == (3,) and 'ws' in c['modes']}
    assert {(n + 15) // 16 <= 4 for n in fused} == {True, False} and any(4 < (n + 15) // 16 <= 8 for n in fused) \
        and any((n + 15) // 16 > 13 for n in fused) and any(c['ns'] == (21, 201) and c['B'] > hp.SWITCH for c in hp.CASES)
    assert {len(c['forms']) for c in hp.CASES} >= {1, 2, 3, 4, 5, 6} and {c['nflags'] for c in hp.CASES} == {0, 1, 3}
    for pos in range(4):                                    # every form in every position
        assert {by['layout_rot%d' % r]['forms'][pos] for r in range(4)} == {0, 1, 2, 3}
    rows = hp.sample_rows(40000)
    assert set(range(64)) <= set(rows) and set(range(39936, 40000)) <= set(rows)
    assert set(range(hp.SWITCH - 64, hp.SWITCH + 64)) <= set(rows) and len(rows) == 64 * 4 + 200
    assert len(hp.sample_rows(hp.SWITCH + 1)) == 64 + 65 + 200               # the last rows lie inside the switch's 128
    k = hp.build_case(by['scaled_wide_aux'])
    se = k['aux'][k['targets'][1].aux_off:][:130]
    assert se.min() == 1.0 and se.max() == 1e6


@pytest.mark.parametrize('name', hp.CASE_NAMES)
def test_plain_fp64_numpy_stays_inside_the_bounds(name):
    """If this fails the case is ill-posed (or the derivation misses a term): change the case, not the bound."""
    k = hp.build_case(hp.CASES[hp.CASE_NAMES.index(name)])
    ref = hp.reference(k)
    keep = ~np.isin(k['rows'], k['poisoned'])
    assert np.isfinite(ref[0][keep].astype(float)).all() and np.isfinite(ref[2][keep].astype(float)).all()
    rl, rm, msg = hp.judge(k, *_scatter(k, *plain_fp64(k, k['rows'])), ref=ref)
    print('HP-RATIO fp64-numpy %s forms=%s logL=%.3f misfit=%.3f' % (name, k['case']['forms'], rl, rm))
    assert msg is None, msg
    failed = (ref[2] == 0) & keep
    if k['case']['failed'] or k['case']['obs'] == 'oob':
        assert failed.any() and np.all(ref[0][failed] == -1e15)


def test_bounds_are_not_vacuous():
    """The gap the old atol = 1e-9 left open: one dropped column of a 201-point dense target with residuals of
    1e-3 moves logL by ~1e-6 * |R^-1| / sigma^2 -- thousands of times the derived bound."""
    k = hp.build_case(hp._case('dropped_column', 16, [3], [201], dense='pinv0.98'))
    k['out'][:] = k['yobs'][0] + 1e-3 * np.random.RandomState(1).standard_normal(k['out'].shape)
    logL, mis = plain_fp64(k, k['rows'])
    assert hp.judge(k, logL, mis)[2] is None
    cut = dict(k, out=k['out'].copy())
    cut['out'][:, 200] = k['yobs'][0, 200]                   # the last column contributes nothing
    wrong = plain_fp64(cut, k['rows'])[0]
    rl, _, msg = hp.judge(k, wrong, mis)
    assert msg is not None and rl > 1e3
