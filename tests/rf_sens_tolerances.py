"""Steps and tolerances of the receiver-function sensitivity kernels (bayhunter_amd/csrc/rf_sens_core.h), measured on
the host twin (tests/hostsim/rf_sens_sim.cpp) against the longdouble reference (tests/rf_sens_ref.py).

THE ERROR of a kind on a case: max over samples and layers of |K_twin - K_ref|, relative to max|K_ref| of that kind and
model (errors()).  Entries the reference flags as not differentiable are left out (none on either list).

THE SWEEP (python tests/rf_sens_tolerances.py): every kind's relative step from 2^-14 to 2^-23, worst error over
rf_sens_cases.CASES without the half-space alone (whose trace, and so K, is NaN: 0 / 0 in the spectral division, in the
reference as in the library).  Too large a step leaves the r^2 truncation term, too small a one divides the trace's
rounding by it; the thickness has the shallowest minimum because earth flattening forms a layer's thickness as a
difference of two depths of tens of km (rf_phase1_layer), which costs the trace three digits in h.  The library's steps
are the minima: SWEEP[kind][log2 r], STEPS_LOG2.

MEASURED: the worst error per kind over CASES at the library's steps; the asserted tolerance is twice that (the sweep's
minimum is flat within a factor of about two between neighbouring powers of two).  REFERENCE_OWN: the reference's
estimate of its own error on the same list, relative in the same way -- at least four times below MEASURED.
OFFLIST_MEASURED: the same measurement on rf_sens_cases.OFFLIST, on which nothing was tuned, asserted at the same margin
over its own worst.  IDENTITY_MEASURED: scaling every density by one factor leaves the trace, so
sum_i rho_i K_rho,i(t) = 0; the residual's maximum over samples relative to max|rho K_rho| over CASES.
"""
import numpy as np

KINDS = ('h', 'vp', 'vs', 'rho')
STEPS_LOG2 = {'h': -17, 'vp': -19, 'vs': -20, 'rho': -17}
MARGIN = 2.0

#        log2 r:    -14        -15        -16        -17        -18        -19        -20        -21        -22        -23
SWEEP = {
    'h':   [1.046e-06, 2.615e-07, 6.457e-08, 5.602e-08, 1.131e-07, 2.315e-07, 7.162e-07, 6.650e-07, 2.848e-06, 4.636e-06],
    'vp':  [3.841e-07, 9.604e-08, 2.401e-08, 6.000e-09, 1.502e-09, 6.144e-10, 1.365e-09, 3.186e-09, 7.477e-09, 9.644e-09],
    'vs':  [1.090e-06, 2.725e-07, 6.812e-08, 1.703e-08, 4.259e-09, 1.090e-09, 2.964e-10, 6.798e-10, 1.266e-09, 1.741e-09],
    'rho': [3.595e-09, 9.009e-10, 2.242e-10, 5.968e-11, 1.093e-10, 2.391e-10, 3.436e-10, 7.763e-10, 1.235e-09, 4.151e-09],
}
SWEEP_LOG2 = list(range(-14, -24, -1))

MEASURED = {'h': 5.602e-08, 'vp': 6.144e-10, 'vs': 2.964e-10, 'rho': 5.968e-11}
REFERENCE_OWN = {'h': 2.012e-10, 'vp': 2.345e-11, 'vs': 6.651e-11, 'rho': 2.536e-13}
OFFLIST_MEASURED = {'h': 5.364e-08, 'vp': 3.631e-10, 'vs': 8.665e-10, 'rho': 3.481e-11}     # (the reference's own: <= 2.3e-10)
IDENTITY_MEASURED = 9.339e-11


def tolerance(kind):
    return MARGIN * MEASURED[kind]


def offlist_bound(kind):
    return MARGIN * OFFLIST_MEASURED[kind]


def identity_tolerance():
    return MARGIN * IDENTITY_MEASURED


def errors(K, R):
    """({kind: error of the twin's K}, {kind: the reference's own error}, entries left out) against R, a dict of
    rf_sens_ref.kernels; both relative to max|K_ref| of the kind."""
    Kr, own, keep = R['K'].astype(np.float64), R['own'].astype(np.float64), ~R['flagged']
    n = Kr.shape[2]
    assert K.shape[0] == Kr.shape[0] and np.array_equal(np.isnan(K[:, :, :n]), np.isnan(Kr))
    err, ref = {}, {}
    for k, kind in enumerate(KINDS):
        scale = np.abs(Kr[:, k]).max()
        d = np.where(keep[:, k], np.abs(K[:, k, :n] - Kr[:, k]), 0.0)
        err[kind] = float(d.max() / scale) if scale > 0 else float(d.max())
        ref[kind] = float(np.where(keep[:, k], own[:, k], 0.0).max() / scale) if scale > 0 else 0.0
    return err, ref, int((~keep).sum())


def identity_residual(K, rho):
    """max_t |sum_i rho_i K_rho,i(t)| / max|rho K_rho|"""
    w = K[:, 3, :len(rho)] * np.asarray(rho)[None, :]
    return float(np.abs(w.sum(axis=1)).max() / np.abs(w).max())


def measure(twin, keys, steps=None):
    """worst errors() per kind over the keys of rf_sens_cases (CASES entries or OFFLIST names)"""
    import rf_sens_cases as rc
    refs = rc.references(keys)
    worst, own = dict.fromkeys(KINDS, 0.0), dict.fromkeys(KINDS, 0.0)
    for key in keys:
        model, par = rc.OFFLIST[key] if key in rc.OFFLIST else (rc.MODELS[key[0]], rc.params(key[1], key[2]))
        K, _ = twin.row(*model, par, steps=steps)
        e, o, _ = errors(K, refs[key])
        for k in KINDS:
            worst[k], own[k] = max(worst[k], e[k]), max(own[k], o[k])
    return worst, own


if __name__ == '__main__':
    import rf_sens_cases as rc
    twin = rc.load_sim()
    cases = [c for c in rc.CASES if c[0] != 'L1']
    print('flagged', rc.reference_flags(cases), rc.reference_flags(list(rc.OFFLIST)))
    for p in SWEEP_LOG2:
        w, _ = measure(twin, cases, steps=[2.0 ** p] * 4)
        print(p, ' '.join('%.3e' % w[k] for k in KINDS))
    w, o = measure(twin, cases)
    print('MEASURED', {k: float('%.3e' % v) for k, v in w.items()})
    print('REFERENCE_OWN', {k: float('%.3e' % v) for k, v in o.items()})
    w, o = measure(twin, list(rc.OFFLIST))
    print('OFFLIST_MEASURED', {k: float('%.3e' % v) for k, v in w.items()}, 'own', o)
    print('IDENTITY_MEASURED %.3e' % max(identity_residual(twin.row(*rc.MODELS[c[0]], rc.params(c[1], c[2]))[0], rc.MODELS[c[0]][3])
                                         for c in cases))
