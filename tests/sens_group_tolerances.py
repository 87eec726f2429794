"""Measured errors of the group-velocity sensitivity kernels' host twin (tests/hostsim/sens_group_sim.cpp) against the
longdouble reference (tests/sens_group_ref.py) over sensitivity_cases.MODELS x PERIODS x both wave types (6 models, 60
(model, wave, period) triples, every slot), and what tests/test_sens_group.py asserts from them.

Error of K^U: relative to max |K^U| over the layers of that (model, period, kind).  Error of U and dU/dT: relative.

    python tests/sens_group_tolerances.py          runs the sweep and the measurements again and prints the tables

The step r_g of the central difference of K^c over T (sens_group_core.h: SENS_GROUP_RG) was swept over powers of two on
the twin with everything else as the library has it.  SWEEP: exponent -> worst error of (K^U of any kind, U, dU/dT).
Too large a step loses to truncation (the error falls by 4 per halving); too small a one to the phase kernels' own
error, which the difference divides by 2 r_g (K^U), and to the roots' rounding over r_g^2 (dU/dT).  U does not depend on
r_g: it is formed from the centre root alone.
"""
RG_LOG2 = -12

SWEEP = {
    6: (1.08e-02, 1.39e-10, 3.07e-03),
    7: (2.70e-03, 1.39e-10, 7.68e-04),
    8: (6.76e-04, 1.39e-10, 1.92e-04),
    9: (1.68e-04, 1.39e-10, 4.80e-05),
    10: (4.26e-05, 1.39e-10, 1.20e-05),
    11: (9.31e-06, 1.39e-10, 3.08e-06),
    12: (6.02e-06, 1.39e-10, 5.77e-07),
    13: (6.14e-06, 1.39e-10, 6.73e-07),
    14: (1.74e-05, 1.39e-10, 5.05e-06),
    15: (3.14e-05, 1.39e-10, 1.28e-05),
    16: (2.61e-04, 1.39e-10, 8.31e-05),
}
# (2^-12 has the smallest error of K^U and of dU/dT)

# worst errors of the twin at RG_LOG2, per kind of K^U, U and dU/dT
MEASURED = {'U': 1.39e-10, 'dU_dT': 5.77e-07, 'h': 7.83e-07, 'vp': 6.02e-06, 'vs': 6.03e-07, 'rho': 1.29e-06}
# the reference's own error estimates on the same scale (|D(2^-16) - D(2^-15)|), worst over the same list
REFERENCE_OWN = {'U': 0.0, 'dU_dT': 4.48e-08, 'h': 4.26e-07, 'vp': 1.31e-08, 'vs': 1.44e-08, 'rho': 6.18e-08}
# (every bound of tolerance() below is its first term: twice MEASURED is above the reference's estimate for each)


def tolerance(what):
    """Twice the measured worst error: the case list is fixed and the twin deterministic, so the factor only absorbs a
    host libm that differs (sqrt and log are the host's).  Never below the reference's own error estimate."""
    return max(2.0 * MEASURED[what], REFERENCE_OWN[what])


# Scaling identities on the twin, residual over the sum of the absolute terms, worst over the same list:
#   'rho'   sum_i rho_i K^U_rho,i = 0
#   'v'     sum_i (vp_i K^U_vp,i + vs_i K^U_vs,i) + sum_i h_i K^U_h,i = U
#   'h'     sum_i h_i K^U_h,i + T dU/dT = 0
IDENTITY_MEASURED = {'rho': 4.02e-07, 'v': 5.22e-07, 'h': 3.43e-07}


def identity_tolerance(which):
    return 2.0 * IDENTITY_MEASURED[which]


# T^2 |c_TT| / c, the curvature the side roots' acceptance window is derived from (sens_group_core.h: SENS_GROUP_KAPPA),
# worst on the twin.  KAPPA_MEASURED: over MODELS x PERIODS, OFFLIST x OFFLIST_PERIODS and the CROSSINGS periods, both
# wave types -- a mild list.  KAPPA_DRAWN: over bayhunter_amd.synthetic.draw_models(16384, 10, seed=1) and
# draw_models(16384, (2, 31), seed=17) (vs increasing downward), 21 periods linspace(1, 41, 21), per wave type; the
# largest values belong to a slow top layer of 10 .. 25 km over fast rock at 33 .. 41 s, where U is about half of c.
# With the window of KAPPA_BOUND none of the (model, period) pairs of those draws that the phase pass serves is without
# a group value.  DRAWN_LOST: models of draw_models(3072, 10, seed=1) -> the period index (of those 21) that a window of
# 4 r_g^2 (a bound of 8) rejected for Rayleigh waves, kappa 8.1 .. 10.3 there; test_sens_group keeps them served.
KAPPA_MEASURED = 0.593
KAPPA_DRAWN = {'rayleigh': 12.5, 'love': 4.03}
KAPPA_BOUND = 64.0
DRAWN_LOST = {28: 20, 45: 20, 90: 17, 492: 17, 704: 19, 1691: 20, 2266: 17, 2717: 17, 2833: 16, 2907: 6}

# Off the list and at the crossings: measured, reported, not asserted.  Worst errors of the twin
# against the reference on the slots of test_sensitivity._subset (Love waves: every slot).
OFFLIST_MEASURED = {'U': 2.08e-09, 'dU_dT': 6.01e-06, 'h': 5.57e-06, 'vp': 1.59e-05, 'vs': 9.03e-06, 'rho': 4.41e-05}
CROSSING_MEASURED = {'U': 1.32e-06, 'dU_dT': 8.14e-04, 'h': 2.03e-05, 'vp': 1.30e-06, 'vs': 1.72e-06, 'rho': 1.69e-06}
# (off the list the worst is lvz23, Rayleigh, 20 s, where the phase kernels themselves are off by 5e-08
# (sensitivity_tolerances.LVZ23_MEASURED) and the difference over T divides that by 2 r_g = 2^-11.  With c on a layer's
# vs the phase pass loses up to 4e-05 of K_h and 8e-06 of dc/dT (sensitivity_tolerances.CROSSING_MEASURED) in a way that
# scatters from period to period, and the difference over T could lose 2048 times that; measured at the 23 recorded
# crossing periods K^U loses 2e-05 at the worst: T+ and T- lie 2^-12 T off the crossing, where the phase kernels are
# whole again, and only the centre term carries the loss.  dU/dT takes the roots' 1e-11 over r_g^2: 8e-04 at the worst.)


# ---- the measurements ------------------------------------------------------------------------------------------------
KINDS = ('h', 'vp', 'vs', 'rho')


def _kscale(K):
    import numpy as np
    s = np.abs(K).max(axis=-1)
    return np.where(s > 0, s, 1.0)


def _ref_task(args):
    import sens_group_ref as gr
    m, T, c0, wave, slots = args
    return gr.kernels(*m, T, c0, wave, slots)


def errors(t, k, r):
    """Twin dict t at period index k against the reference dict r: (errors, the reference's own estimates) by what."""
    import numpy as np
    scale = _kscale(t['K'][k])
    e = dict(U=float(abs(t['U'][k] - r['U']) / r['U']), dU_dT=float(abs(t['dU_dT'][k] - r['dU_dT']) / abs(r['dU_dT'])))
    own = dict(U=0.0, dU_dT=float(r['dU_dT_err'] / abs(r['dU_dT'])))
    with np.errstate(invalid='ignore'):
        for i, kind in enumerate(KINDS):
            if np.isnan(r['K'][i].astype(np.float64)).all():
                e[kind] = own[kind] = 0.0
                continue
            e[kind] = float(np.nanmax(np.abs(t['K'][k, i] - r['K'][i])) / scale[i])
            own[kind] = float(np.nanmax(r['K_err'][i]) / scale[i])
    return e, own


def identities(m, t, periods):
    """Residuals of the three identities over the sum of the absolute terms, worst over the periods."""
    import numpy as np
    h, vp, vs, rho = m
    worst = dict(rho=0.0, v=0.0, h=0.0)
    for k, T in enumerate(periods):
        K, U, d = t['K'][k], t['U'][k], t['dU_dT'][k]
        terms = dict(rho=rho * K[3], v=np.concatenate([vp * K[1], vs * K[2], h * K[0], [-U]]),
                     h=np.concatenate([h * K[0], [T * d]]))
        for key, x in terms.items():
            worst[key] = max(worst[key], abs(x.sum()) / np.abs(x).sum())
    return worst


def kappa(t, periods):
    """T^2 |c_TT| / c from the twin's dU/dT, U, c and dc/dT: D' = (c_T / D - dU/dT) D^2 / c, then c_TT out of D'."""
    import numpy as np
    T, c, cT, U, dU = (np.asarray(x) for x in (periods, t['c'], t['dc_dT'], t['U'], t['dU_dT']))
    D = 1.0 + T * cT / c
    Dp = (cT / D - dU) * D * D / c
    cTT = (Dp - cT / c + T * cT * cT / (c * c)) * c / T
    return float(np.max(T * T * np.abs(cTT) / c))


def main():
    import multiprocessing as mp
    import numpy as np
    import sensitivity_cases as sc
    import sensitivity_ref as ref
    import sens_group_cases as gc
    tw = gc.load_sim()
    pool = mp.Pool(min(16, mp.cpu_count()))
    # the tuning list
    tasks, twins = [], {}
    for name, wave in sc.CASES:
        m = sc.MODELS[name]
        t = twins[(name, wave)] = tw.sensitivity(*m, sc.PERIODS, wave)
        tasks += [(m, T, c0, wave, None) for T, c0 in zip(sc.PERIODS, t['c0'])]
    refs = pool.map(_ref_task, tasks, chunksize=1)
    R = {case: refs[5 * i:5 * i + 5] for i, case in enumerate(sc.CASES)}
    what = ('U', 'dU_dT') + KINDS
    print('SWEEP = {')
    best = {}
    for p in range(6, 17):
        worst = dict.fromkeys(what, 0.0)
        for (name, wave), rs in R.items():
            t = tw.sensitivity(*sc.MODELS[name], sc.PERIODS, wave, rg=2.0 ** -p)
            for k, r in enumerate(rs):
                e, _ = errors(t, k, r)
                worst = {w: max(worst[w], e[w]) for w in what}
        best[p] = worst
        print('    %d: (%.2e, %.2e, %.2e),' % (p, max(worst[k] for k in KINDS), worst['U'], worst['dU_dT']))
    print('}')
    print('MEASURED =', {w: float('%.2e' % v) for w, v in best[-RG_LOG2].items()})
    own = dict.fromkeys(what, 0.0)
    ident = dict(rho=0.0, v=0.0, h=0.0)
    kap = 0.0
    for (name, wave), rs in R.items():
        t = twins[(name, wave)]
        for k, r in enumerate(rs):
            own = {w: max(own[w], errors(t, k, r)[1][w]) for w in what}
        i = identities(ref.round_model(*sc.MODELS[name]), t, sc.PERIODS)
        ident = {w: max(ident[w], i[w]) for w in ident}
        kap = max(kap, kappa(t, sc.PERIODS))
    print('REFERENCE_OWN =', {w: float('%.2e' % v) for w, v in own.items()})
    print('IDENTITY_MEASURED =', {w: float('%.2e' % v) for w, v in ident.items()})
    # off the list and at the crossings (reported, not asserted)
    ts = __import__('test_sensitivity')
    tasks, keys = [], []
    for name, wave in sc.OFFLIST_CASES:
        m = sc.OFFLIST[name]
        t = twins[('off', name, wave)] = tw.sensitivity(*m, sc.OFFLIST_PERIODS, wave)
        kap = max(kap, kappa(t, sc.OFFLIST_PERIODS))
        for k, (T, c0) in enumerate(zip(sc.OFFLIST_PERIODS, t['c0'])):
            slots = None if wave == 'love' else ts._subset(t['K'][k], len(m[0]))
            tasks.append((m, T, c0, wave, slots))
            keys.append((('off', name, wave), k))
    for (name, wave, i), T in sorted(sc.CROSSINGS.items()):
        m = sc.MODELS[name]
        t = twins[('x', name, wave, i)] = tw.sensitivity(*m, np.array([T]), wave)
        kap = max(kap, kappa(t, np.array([T])))
        slots = None if wave == 'love' else ts._subset(t['K'][0], len(m[0]), (i,))
        tasks.append((m, T, t['c0'][0], wave, slots))
        keys.append((('x', name, wave, i), 0))
    refs = pool.map(_ref_task, tasks, chunksize=1)
    off, cross = dict.fromkeys(what, 0.0), dict.fromkeys(what, 0.0)
    for (key, k), r in zip(keys, refs):
        e, _ = errors(twins[key], k, r)
        into = off if key[0] == 'off' else cross
        for w in what:
            into[w] = max(into[w], e[w])
        print('   ', key, k, {w: float('%.1e' % v) for w, v in e.items()})
    print('KAPPA_MEASURED = %.3g' % kap)
    print('OFFLIST_MEASURED =', {w: float('%.2e' % v) for w, v in off.items()})
    print('CROSSING_MEASURED =', {w: float('%.2e' % v) for w, v in cross.items()})


if __name__ == '__main__':
    main()
