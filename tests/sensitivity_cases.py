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
