"""Models and the host twin shared by tests/test_ellipticity.py and tests/test_gpu_ellipticity.py.

The twin is tests/hostsim/ell_sim.cpp: bayhunter_amd/csrc/ell_core.h compiled with g++ and the device math of
bh_math.h (the flags of conftest's hostsim_devmath build), with the search that supplies the phase velocities.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
SIM_SRCS = [os.path.join(HOSTSIM, 'ell_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                      ('ell_core.h', 'swd_core.h', 'bh_math.h', 'bh_common.h')]
FMA = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []

PER21 = np.linspace(1., 41., 21)
PER60 = np.linspace(0.3, 10., 60)
FORM_TZ, FORM_TR = 0, 1          # ELL_FORM_TZ, ELL_FORM_TR


def stack(n, seed, lvz=False):
    """n layers, Vs rising from about 2 to 4.5 km/s into the half-space (an inverted layer in the middle with lvz),
    Vp/Vs 1.75, the reference's density relation."""
    rng = np.random.RandomState(seed)
    vs = np.sort(np.linspace(2.0, 4.5, n) + rng.uniform(-0.1, 0.1, n))
    if lvz:
        vs[n // 2] *= 0.85
    h = rng.uniform(1.0, 8.0 if n <= 10 else 3.0, n)
    h[-1] = 0.
    vp = vs * 1.75
    return h, vp, vs, vp * 0.32 + 0.77


def sediment():
    """300 m of soft sediment on a crustal stack: between about 1.8 and 3.9 s the fundamental mode is prograde (the
    ratio is negative), with a zero of the horizontal and a zero of the vertical displacement at the window's ends."""
    return (np.array([0.3, 1.5, 10., 20., 0.]), np.array([1.6, 3.4, 5.6, 6.5, 7.9]), np.array([0.35, 1.8, 3.2, 3.7, 4.4]),
            np.array([1.8, 2.3, 2.6, 2.9, 3.3]))


# name -> (model, periods); every case is run with flsph 0 and 1
CASES = {'L2': (stack(2, 2), PER21), 'L3': (stack(3, 3), PER21), 'L5': (stack(5, 5), PER21), 'L10': (stack(10, 10), PER21),
         'L31': (stack(31, 31), PER21), 'lvz': (stack(10, 11, lvz=True), PER21), 'sediment': (sediment(), PER60)}


def load_sim():
    so = os.path.join(HOSTSIM, 'libell_sim.so')
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SIM_SRCS):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + FMA + ['-o', so, SIM_SRCS[0]],
                       check=True)
    lib = C.CDLL(so)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    lib.es_ell_row.restype = None
    lib.es_ell_row.argtypes = [dp, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int,
                               dp]
    lib.es_ellipticity.restype = C.c_int
    lib.es_ellipticity.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp]
    return Twin(lib)


class Twin(object):
    def __init__(self, lib):
        self.lib = lib

    def ellipticity(self, h, vp, vs, rho, periods, flsph=0, absolute=False):
        """es_ellipticity: (ell, c, err) of one model, the layers rounded to real*4."""
        f = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)) for x in (h, vp, vs, rho)]
        t = np.ascontiguousarray(periods, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        ell, cg = np.zeros(t.size), np.zeros(t.size)
        err = self.lib.es_ellipticity(*[x.ctypes.data for x in f], len(f[0]), flsph, t.size, t.ctypes.data_as(dp),
                                      1 if absolute else 0, ell.ctypes.data_as(dp), cg.ctypes.data_as(dp))
        return ell, cg, err

    def row(self, h, vp, vs, rho, periods, c, nlay=None, Lmax=None, flsph=0, err=0, absolute=False, form=FORM_TZ,
            sphere_path=0):
        """es_ell_row: one row of bh_ell_batch from fp64 layers (nlay of them valid) and the phase velocities c."""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (h, vp, vs, rho)]
        t, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (periods, c))
        nlay = len(a[0]) if nlay is None else int(nlay)
        out = np.zeros(t.size)
        self.lib.es_ell_row(*[x.ctypes.data_as(dp) for x in a], nlay, nlay if Lmax is None else int(Lmax), flsph, t.size,
                            t.ctypes.data_as(dp), c.ctypes.data_as(dp), int(err), 1 if absolute else 0, form, sphere_path,
                            out.ctypes.data_as(dp))
        return out
