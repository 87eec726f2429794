"""Measured error of the ellipticity's host twin against tests/ellipticity_ref.py (numpy.longdouble), and the bound
the tests assert.

Measured on the CPU over tests/ellipticity_cases.py: CASES (2, 3, 5, 10 and 31 layers, a low-velocity zone, a sediment
layer with a prograde window; 21 periods each, the sediment case 60), each with flsph 0 and 1: 372 (model, period)
pairs, none of them within 1e-6 c of a zero of the vertical displacement (the cap is 1 %).  The twin is
bayhunter_amd/csrc/ell_core.h built with g++ and the device math of bh_math.h; the error is relative to
max(|ratio|, 1e-3), at the phase velocity the twin's own search returned.

    form                                   worst error     where
    ELL_FORM_TZ   e[3] / (wvno e[2])       8.911e-14       sediment, flat: next to the pole, |ratio| = 151
    ELL_FORM_TR   -wvno e[2] / e[1]        1.006e-02       the same period; 1.2e-05 .. 2.5e-05 on the smooth models

ELL_FORM_TZ is what the library computes: like the reference it eliminates the normal traction, so it is the same
function of c and only rounding separates the two; everywhere but next to the pole the error is 2e-15 .. 5e-15.
ELL_FORM_TR is a different function of c that meets the first at an exact root: its distance is the search's stopping
tolerance (1e-6 c, then the rounding to real*4) times the sensitivity of the ratio to c.
"""
WORST_TZ = 8.911290590599154e-14      # measured, see above
WORST_TR = 1.0063233701374021e-02     # measured; recorded, asserted nowhere
LIBM_FACTOR = 4.0                     # the twin's sqrt/log/pow are the host libm's, the device's are ocml's
ELL_RTOL = LIBM_FACTOR * WORST_TZ     # relative to max(|ratio|, ELL_FLOOR)
ELL_FLOOR = 1.0e-3
SEARCH_RTOL = 1.0e-6 + 2.0 ** -23     # c against the exact root: nevill's stopping rule, then the rounding to real*4
EXCLUDED_CAP = 0.01                   # share of the cases that may lie within 1e-6 c of a zero of Uz
