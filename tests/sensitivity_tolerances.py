"""Measured errors of the sensitivity kernels' host twin (tests/hostsim/sens_sim.cpp) against the longdouble reference
(tests/sensitivity_ref.py) over sensitivity_cases.CASES (6 models x 2 wave types x 5 periods), and what
tests/test_sensitivity.py asserts from them.

Error of K: relative to max |K| over the layers of that (model, period, kind).  Error of c and dc/dT: relative.

The steps of the central differences (sens_core.h: sens_steps) were chosen by coordinate descent on the twin, each
kind swept over 2^-14 .. 2^-26 with the others held, until a round changed nothing (three rounds from 2^-18, 2^-17,
2^-16, 2^-17, 2^-14).  SWEEP is the last round: kind -> {exponent: worst error of the values the step governs} -- for
c every K and dc/dT, for T dc/dT, for h K_h, for the velocities K_vp and K_vs, for the density K_rho.  Too large a step
loses to truncation (the error falls by 4 per halving), too small a one to the rounding error of F (about 1e-15 / r).
"""
STEPS_LOG2 = {'c': -20, 'T': -16, 'h': -16, 'v': -20, 'rho': -20}

SWEEP = {
    'c': {14: 5.04e-06, 15: 1.26e-06, 16: 3.15e-07, 17: 7.88e-08, 18: 1.97e-08, 19: 5.22e-09, 20: 4.01e-09, 21: 4.01e-09,
          22: 4.68e-09, 23: 4.32e-09, 24: 4.15e-09, 25: 9.61e-09, 26: 1.60e-08},
    'T': {14: 1.37e-08, 15: 4.54e-09, 16: 1.70e-09, 17: 8.76e-09, 18: 8.29e-09, 19: 7.84e-08, 20: 1.01e-07, 21: 1.87e-08,
          22: 2.91e-07, 23: 1.52e-06, 24: 3.91e-07, 25: 2.68e-06, 26: 1.32e-05},
    'h': {14: 2.52e-08, 15: 6.31e-09, 16: 4.01e-09, 17: 4.01e-09, 18: 4.01e-09, 19: 4.77e-09, 20: 4.43e-09, 21: 1.26e-08,
          22: 5.96e-08, 23: 2.72e-08, 24: 1.06e-07, 25: 1.18e-07, 26: 3.80e-07},
    'v': {14: 5.27e-06, 15: 1.32e-06, 16: 3.28e-07, 17: 8.12e-08, 18: 1.94e-08, 19: 3.94e-09, 20: 6.04e-10, 21: 1.87e-09,
          22: 3.53e-09, 23: 6.03e-09, 24: 1.78e-08, 25: 2.01e-08, 26: 3.37e-08},
    'rho': {14: 3.63e-09, 15: 1.37e-09, 16: 1.37e-09, 17: 1.37e-09, 18: 1.35e-09, 19: 1.38e-09, 20: 1.24e-09, 21: 1.31e-09,
            22: 2.24e-09, 23: 4.67e-09, 24: 1.53e-08, 25: 1.38e-08, 26: 3.74e-08},
}
# (for c the minimum is flat between 2^-20 and 2^-21, where the worst value is K_h's 4.01e-09 at either; 2^-20 has the
# smaller error in K_vs and K_rho: 4.2e-10 and 1.2e-09 against 8.8e-10 and 1.2e-09)

# worst errors of the twin at STEPS_LOG2
MEASURED = {'c': 4.50e-16, 'dc_dT': 1.70e-09, 'h': 4.01e-09, 'vp': 6.04e-10, 'vs': 4.20e-10, 'rho': 1.24e-09}
# the reference's own error estimates (|D(2^-18) - D(2^-17)|, the same scale), worst over sensitivity_cases.CASES and
# over the second list, sensitivity_cases.OFFLIST without lvz23 (every slot, both wave types, 5 and 2 periods).  On CASES
# alone they were dc_dT 8.66e-10, vp 3.17e-10, vs 5.93e-10; draw0 raises them: dc_dT and vp (Rayleigh, 2 s), vs (Love,
# 2 s: 1.62e-09).  10 x this was the binding term of tolerance() for dc_dT, h, vp, vs and rho already, and is the only
# way in which tolerance() has moved since the steps were tuned: dc_dT 8.7e-09 -> 9.1e-09, vp 3.2e-09 -> 3.4e-09,
# vs 5.9e-09 -> 1.6e-08; c (4 x MEASURED), h and rho are as they were.  That is the reference's resolution, not the
# twin's error: MEASURED is untouched, and the twin's worst errors on the second list are below it but for vp
# (1.5e-09 at L8x18).
REFERENCE_OWN = {'c': 1.0e-17, 'dc_dT': 9.09e-10, 'h': 2.49e-09, 'vp': 3.41e-10, 'vs': 1.63e-09, 'rho': 1.58e-09}


def tolerance(what):
    """4 x the measured worst error (the margin for models outside the list), never below 10 x the reference's own
    recorded error estimate."""
    return max(4.0 * MEASURED[what], 10.0 * REFERENCE_OWN[what])


# lvz23 (tests/golden/lvz_worst_cases.npz, case 2 row 0: 23 layers whose vs jumps between 2.1 and 5.0 km/s) is outside
# tolerance() for Rayleigh waves, and keeps a table of its own, against the longdouble reference over every slot at 2 s
# and 20 s.  At 20 s every kind and dc/dT are off by the same 4.9e-08: the common factor 1 / F_c, whose central
# difference over c (1 +- 2^-20) is not converged in a stack whose period equation bends this fast; the polished c is
# 5.5e-15 from the reference's root.  At 2 s the reference's own estimate for K_rho is 3.5e-08.  Love waves stay inside
# tolerance().  The second entry of each pair is the reference's own estimate.  The search's c0 at 20 s depends on
# whether 2 s was searched before it in the same call, and the polished c and F_c with it: both periods in one call, as
# test_sensitivity runs them, give c 2.8e-14, dc/dT 2.3e-08 and K 1.1e-08 on the slots compared; the table has the worse.
LVZ23_MEASURED = {'c': (2.80e-14, 1.0e-17), 'dc_dT': (3.68e-08, 2.80e-10), 'h': (4.88e-08, 7.47e-10),
                  'vp': (5.60e-08, 3.32e-10), 'vs': (4.90e-08, 1.46e-10), 'rho': (4.84e-08, 3.46e-08)}


def lvz23_tolerance(what):
    """tolerance(), or 4 x what lvz23 measures where that is more (and 10 x the reference's estimate there)."""
    return max(tolerance(what), 4.0 * LVZ23_MEASURED[what][0], 10.0 * LVZ23_MEASURED[what][1])


# Where c crosses the vs of a layer (sensitivity_cases.CROSSINGS: every reachable finite layer of L3, L8 and lvz, both
# wave types, 23 crossings) the layer step changes from its trigonometric to its hyperbolic form, and on the hyperbolic
# side swd_var / swd_love_layer form e^-q sinh q as (1 - e^-2q) / 2, which keeps an absolute error of 2^-54 whatever q
# is: relative 6e-17 / q, with q = d k sqrt(2 |c / vs - 1|) for small distances.  (The longdouble reference has no such
# loss: its own estimates below are what they are elsewhere.)  It reaches the result wherever an evaluation of F falls
# next to the crossing: at c = vs itself (the polish and the slots), and where c is one step of the central difference
# over c or over the velocity, 2^-20, away from vs -- then F at c (1 -+ 2^-20), or at vs (1 +- 2^-20), sits on it.
# Worst errors of the twin against the longdouble reference over the 23 crossings at c / vs - 1 = 0, +-2^-24 and
# +-2^-20, the worse of two measurements: every slot at the periods where a bisection on the twin's polished c ends
# (|c / vs - 1| up to 9e-12), and the slots test_sensitivity compares at the recorded periods (|c / vs - 1| <= 4e-14).
# How bad a value is depends on how close an evaluation falls, so it scatters from period to period: at distance 0 the
# first measurement had dc/dT 8.6e-07 and K_h 9.0e-07, the second c 1.2e-12.
#               distance 0      +-2^-24     +-2^-20
#     c         9.2e-12         1.4e-14     3.1e-15
#     dc/dT     7.6e-06         7.1e-09     1.4e-06
#     K_h       4.2e-05         5.0e-09     1.4e-06
#     K_vp      1.7e-09         2.4e-09     1.4e-06
#     K_vs      3.8e-09         7.8e-09     7.0e-04    (the crossed layer's own slot: its perturbed vs is c)
#     K_rho     1.6e-09         2.1e-09     1.4e-06
# and at +-2^-16 and +-2^-12: c 1.1e-15, dc/dT 9.0e-10, K_h 6.1e-10, K_vp 9.5e-10, K_vs 2.1e-09, K_rho 8.1e-10 -- inside
# tolerance().  The reference's own estimates over all of these: dc/dT 1.2e-10, h 5.1e-10, vp 2.7e-10, vs 1.5e-10,
# rho 7.9e-11.
CROSSING_MEASURED = {'c': 9.18e-12, 'dc_dT': 7.55e-06, 'h': 4.17e-05, 'vp': 1.44e-06, 'vs': 6.98e-04, 'rho': 1.44e-06}
# |c / vs - 1| from which tolerance() holds again (the smallest measured distance at which it does; between 2^-20 and
# 2^-16 nothing was measured)
CROSSING_REACH = 2.0 ** -16


def crossing_tolerance(what):
    """Within CROSSING_REACH of a layer's vs: 4 x the worst error measured there -- the margin tolerance() uses, for
    the same reason: the crossings of other models."""
    return max(tolerance(what), 4.0 * CROSSING_MEASURED[what])


# Scaling identities, residual over the sum of the absolute terms, worst over the cases: measured on the twin
#   'rho'   sum_i rho_i K_rho,i = 0
#   'v'     sum_i (vp_i K_vp,i + vs_i K_vs,i) - T dc/dT = c
#   'h'     sum_i h_i K_h,i + T dc/dT = 0
IDENTITY_MEASURED = {'rho': 2.42e-10, 'v': 1.38e-10, 'h': 4.25e-10}
# (the reference itself leaves 1.2e-09, 1.5e-12 and 2.2e-11)
# the same residuals, worst over 64 seeded draws of 2-31 layers (draw_models(64, (2, 31), seed=17, sorted_vs=True)), both
# wave types, sensitivity_cases.PERIODS: measured on the twin, asserted within identity_tolerance() of the six models
# there only for 'v': 'rho' (draw 46, 21 layers, Rayleigh, 3 s) and 'h' (draw 22, 8 layers, Rayleigh, 3 s) exceed it,
# inside what tolerance()'s 4 x MEASURED per K allows a sum over the layers (the test states that bound)
IDENTITY_MEASURED_DRAWS = {'rho': 2.55e-09, 'v': 4.52e-10, 'h': 1.79e-09}
# Where T |dc/dT| < IDENTITY_FLOOR c the wave is not dispersive and the terms of the 'rho' and 'h' identities are
# rounding themselves (test_scaling_identities_over_many_drawn_models); there the residual is taken over
# IDENTITY_FLOOR c.  The floor: the terms' absolute error is the difference quotients', 3e-12 c in that example, so a
# residual of identity_tolerance, 1e-09 of the terms, needs terms of 3e-03 c; the floor is three times that.
IDENTITY_FLOOR = 1.0e-2
IDENTITY_LEFT_OUT = 42                  # of the 2 x 64 x 5 (model, period) pairs


def identity_tolerance(which):
    return 4.0 * IDENTITY_MEASURED[which]


# group velocity c / (1 + (T / c) dc/dT) of the twin against the reference's (roots at T (1 +- 2^-18)), relative,
# worst over L2, L3, lvz and thin, both wave types
GROUP_MEASURED = 1.21e-10
GROUP_RTOL = 4.0 * GROUP_MEASURED

# the polish: a stored c further than this (relative) from the polished root is another root (sens_core.h)
ACCEPT = 2.0e-6
