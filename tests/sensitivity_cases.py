"""Models, periods and the host twin shared by tests/test_sensitivity.py and tests/test_gpu_sensitivity.py.

The twin is tests/hostsim/sens_sim.cpp: bayhunter_amd/csrc/sens_core.h compiled with g++ and the device math of
bh_math.h (the flags of conftest's hostsim_devmath build), with the search that supplies the phase velocities.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
SIM_SRCS = [os.path.join(HOSTSIM, 'sens_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                       ('sens_core.h', 'swd_core.h', 'bh_math.h', 'bh_common.h')]
FMA = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
WAVES = {'love': 1, 'rayleigh': 2}


def _model(vs, h):
    vs, h = np.asarray(vs, dtype=np.float64), np.asarray(h, dtype=np.float64)
    vp = 1.75 * vs
    return h, vp, vs, 0.77 + 0.32 * vp


# Velocities increasing downward at 2, 3, 7 and 8 layers; a low-velocity zone; a thin (50 m) top layer.
MODELS = {
    'L2': _model([3.2, 4.4], [12., 0.]),
    'L3': _model([2.6, 3.5, 4.4], [4., 18., 0.]),
    'L7': _model([2.2, 2.7, 3.1, 3.4, 3.7, 4.0, 4.5], [1.5, 3., 4., 6., 8., 10., 0.]),
    'L8': _model([2.0, 2.5, 2.9, 3.3, 3.6, 3.8, 4.1, 4.6], [1., 2., 3.5, 5., 6.5, 8., 11., 0.]),
    'lvz': _model([2.8, 3.5, 3.0, 3.8, 4.5], [3., 6., 7., 14., 0.]),
    'thin': _model([1.2, 2.9, 3.6, 4.4], [0.05, 6., 20., 0.]),
}
# Five periods: at the short ones c lies below the vs of the deeper layers (the hyperbolic branch of their layer step),
# at the long ones above the vs of the shallow layers (the trigonometric branch); test_sensitivity checks that both occur.
PERIODS = np.array([3., 7., 14., 25., 45.])
CASES = [(name, wave) for name in MODELS for wave in ('rayleigh', 'love')]

# Rows without a value, by what makes them so: (what, change to the row)
NO_VALUE = ('water', 'flag', 'c_zero', 'c_moved')


# ---- models outside the list the tolerances were tuned on --------------------------------------------------------------------
def deepen(model, n, spread=0.01):
    """`model` cut to n layers: the thickest finite layer (the first of equals) is halved until there are n, then the
    pieces of one original layer get its vs times 1 + spread * (position - 1/2), position (k + 1/2) / pieces from the
    top, so that the result is another model and, for spread below the smallest relative vs step, still increasing
    wherever `model` is.  vp and rho follow vs as in _model."""
    h, owner = list(np.asarray(model[0], dtype=np.float64)), list(range(len(model[0])))
    assert n >= len(h)
    while len(h) < n:
        j = int(np.argmax(h[:-1]))
        h[j:j + 1] = [h[j] / 2, h[j] / 2]
        owner[j:j + 1] = [owner[j], owner[j]]
    owner = np.array(owner)
    vs = np.asarray(model[2], dtype=np.float64)[owner]
    for o in set(owner):
        at = np.nonzero(owner == o)[0]
        vs[at] *= 1.0 + spread * ((np.arange(at.size) + 0.5) / at.size - 0.5)
    return _model(vs, h)


def halve_layer(model, i):
    """Layer i cut into two layers of half its thickness (exact in real*4) with the same vp, vs and rho."""
    out = []
    for k, x in enumerate(model):
        x = list(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))
        x[i:i + 1] = [x[i] / 2, x[i] / 2] if k == 0 else [x[i], x[i]]
        out.append(np.array(x))
    return tuple(out)


def _drawn(row):
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nlay = draw_models(4, (10, 10), seed=5, sorted_vs=True)
    return tuple(x[row, :nlay[row]].copy() for x in (H, VP, VS, RHO))


def _lvz_fixture(case, row):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'lvz_worst_cases.npz'))
    n = int(z['c%d_nl' % case][row])
    return tuple(z['c%d_%s' % (case, k)][row, :n].astype(np.float64) for k in ('H', 'VP', 'VS', 'RHO'))


# The second list, on which no step and no tolerance was tuned: two seeded 10-layer draws (the depth of
# tools/sensitivity_bench.py), L8 cut to 18 layers, and the 23-layer model of tests/golden/lvz_worst_cases.npz (case 2,
# row 0: vs jumps between 2.1 and 5.0 km/s from layer to layer over a half-space of 4.80 km/s, which only one 3 km layer
# of 4.97 km/s exceeds -- none of the fixture's 13 models has a half-space faster than every layer; three have water on
# top).  Two periods each.
OFFLIST = {
    'draw0': _drawn(0),
    'draw1': _drawn(1),
    'L8x18': deepen(MODELS['L8'], 18),
    'lvz23': _lvz_fixture(2, 0),
}
OFFLIST_PERIODS = np.array([2., 20.])
OFFLIST_CASES = [(name, wave) for name in OFFLIST for wave in ('rayleigh', 'love')]


# ---- branch crossings ---------------------------------------------------------------------------------------------------------
def period_at(twin, model, wave, target, lo=0.3, hi=150.0):
    """The period at which the twin's polished c is `target`, by bisection in [lo, hi] (c rises with T there: the caller
    checks the ends).  None when target is not between the ends."""
    def c_of(T):
        r = twin.sensitivity(*model, np.array([T]), wave)
        return r['c'][0] if r['err'] == 0 else np.nan
    clo, chi = c_of(lo), c_of(hi)
    if not (clo < target < chi):
        return None
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if c_of(mid) < target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# Periods at which the twin's polished c equals the real*4 vs of layer i of the model: (model, wave, i) -> T, found with
# period_at and, since the polished c scatters by 1e-12 there, the closest of T (1 + j 2e-14), |j| <= 60, around its
# result (test_sensitivity checks that they still land there).  Every finite layer of L3, L8 and lvz whose vs a
# fundamental mode of 0.3 .. 150 s reaches.
CROSSINGS = {                                               # c / vs - 1 of the twin's polished c
    ('L3', 'rayleigh', 0): 3.106365031876115,               # 1.9e-14
    ('L3', 'rayleigh', 1): 15.856311632649065,              # 4.1e-14
    ('L3', 'love', 1): 11.176906739659756,                  # 0
    ('L8', 'rayleigh', 0): 1.1298063783413355,              # 3.0e-14
    ('L8', 'rayleigh', 1): 3.8000739329604443,              # 4.4e-16
    ('L8', 'rayleigh', 2): 7.636639430141306,               # 1.6e-15
    ('L8', 'rayleigh', 3): 14.035143812324192,              # 1.5e-14
    ('L8', 'rayleigh', 4): 20.15693409653462,               # 7.5e-15
    ('L8', 'rayleigh', 5): 26.442624149820386,              # 2.7e-14
    ('L8', 'rayleigh', 6): 89.88506292908889,               # 2.3e-15
    ('L8', 'love', 1): 2.8434721641243734,                  # 5.6e-15
    ('L8', 'love', 2): 6.209414292554386,                   # 0
    ('L8', 'love', 3): 11.44802595181374,                   # 2.2e-15
    ('L8', 'love', 4): 17.090495870608706,                  # 2.9e-15
    ('L8', 'love', 5): 21.69399449903746,                   # 6.7e-16
    ('L8', 'love', 6): 30.910808278834722,                  # 0
    ('lvz', 'rayleigh', 0): 2.407837374390026,              # 2.5e-14
    ('lvz', 'rayleigh', 1): 18.57665705407409,              # 8.9e-16
    ('lvz', 'rayleigh', 2): 9.691488869320105,              # 6.3e-15
    ('lvz', 'rayleigh', 3): 26.84235627779169,              # 1.6e-15
    ('lvz', 'love', 1): 12.535927041933116,                 # 1.3e-15
    ('lvz', 'love', 2): 2.045798250330698,                  # 6.7e-16
    ('lvz', 'love', 3): 20.848236841826353,                 # 7.1e-15
}
# the distances c / vs - 1 at which the comparison is repeated on either side
CROSSING_DISTANCES = (2.0 ** -24, 2.0 ** -20, 2.0 ** -16, 2.0 ** -12)


def load_sim():
    so = os.path.join(HOSTSIM, 'libsens_sim.so')
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SIM_SRCS):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + FMA + ['-o', so, SIM_SRCS[0]],
                       check=True)
    lib = C.CDLL(so)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    lib.ss_sens_row.restype = None
    lib.ss_sens_row.argtypes = [dp, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, dp, dp, dp, dp]
    lib.ss_sensitivity.restype = C.c_int
    lib.ss_sensitivity.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp]
    return Twin(lib)


class Twin(object):
    def __init__(self, lib):
        self.lib = lib

    def sensitivity(self, h, vp, vs, rho, periods, wave='rayleigh'):
        """ss_sensitivity: dict K [nper][4][n], c, dc_dT, c0 (the search's phase velocities), err; layers real*4."""
        f = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)) for x in (h, vp, vs, rho)]
        t = np.ascontiguousarray(periods, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        n = len(f[0])
        K, c, d, cg = np.zeros((t.size, 4, n)), np.zeros(t.size), np.zeros(t.size), np.zeros(t.size)
        err = self.lib.ss_sensitivity(*[x.ctypes.data for x in f], n, WAVES[wave], t.size, t.ctypes.data_as(dp),
                                      *[x.ctypes.data_as(dp) for x in (K, c, d, cg)])
        return dict(K=K, c=c, dc_dT=d, c0=cg, err=err)

    def row(self, h, vp, vs, rho, periods, c, wave='rayleigh', nlay=None, Lmax=None, err=0, steps=None):
        """ss_sens_row: one row of bh_sens_batch from fp64 layers (nlay of them valid) and the phase velocities c:
        (K [nper][4][Lmax], c_out, dc_dT).  steps: the five relative steps (c, T, h, velocities, density) or None."""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (h, vp, vs, rho)]
        t, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (periods, c))
        nlay = len(a[0]) if nlay is None else int(nlay)
        Lmax = nlay if Lmax is None else int(Lmax)
        assert all(x.size >= min(max(nlay, 1), Lmax) for x in a)
        K, co, d = np.zeros((t.size, 4, Lmax)), np.zeros(t.size), np.zeros(t.size)
        st = None if steps is None else np.ascontiguousarray(steps, dtype=np.float64)
        self.lib.ss_sens_row(*[x.ctypes.data_as(dp) for x in a], nlay, Lmax, WAVES[wave], t.size, t.ctypes.data_as(dp),
                             c.ctypes.data_as(dp), int(err), None if st is None else st.ctypes.data_as(dp),
                             *[x.ctypes.data_as(dp) for x in (K, co, d)])
        return K, co, d
