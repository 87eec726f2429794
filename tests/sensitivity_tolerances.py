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
# the reference's own error estimates (|D(2^-18) - D(2^-17)|, the same scale), worst over the cases
REFERENCE_OWN = {'c': 1.0e-17, 'dc_dT': 8.66e-10, 'h': 2.49e-09, 'vp': 3.17e-10, 'vs': 5.93e-10, 'rho': 1.58e-09}


def tolerance(what):
    """4 x the measured worst error (the margin for models outside the list), never below 10 x the reference's own
    recorded error estimate."""
    return max(4.0 * MEASURED[what], 10.0 * REFERENCE_OWN[what])


# Scaling identities, residual over the sum of the absolute terms, worst over the cases: measured on the twin
#   'rho'   sum_i rho_i K_rho,i = 0
#   'v'     sum_i (vp_i K_vp,i + vs_i K_vs,i) - T dc/dT = c
#   'h'     sum_i h_i K_h,i + T dc/dT = 0
IDENTITY_MEASURED = {'rho': 2.42e-10, 'v': 1.38e-10, 'h': 4.25e-10}
# (the reference itself leaves 1.2e-09, 1.5e-12 and 2.2e-11)


def identity_tolerance(which):
    return 4.0 * IDENTITY_MEASURED[which]


# group velocity c / (1 + (T / c) dc/dT) of the twin against the reference's (roots at T (1 +- 2^-18)), relative,
# worst over L2, L3, lvz and thin, both wave types
GROUP_MEASURED = 1.21e-10
GROUP_RTOL = 4.0 * GROUP_MEASURED

# the polish: a stored c further than this (relative) from the polished root is another root (sens_core.h)
ACCEPT = 2.0e-6
