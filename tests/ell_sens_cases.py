"""The host twin of the ellipticity sensitivity kernels, shared by tests/test_ell_sens.py, tests/test_gpu_ell_sens.py and
tests/ell_sens_tolerances.py.  Models, periods and the rows without a value are sensitivity_cases'.

The twin is tests/hostsim/ell_sens_sim.cpp: bayhunter_amd/csrc/ell_sens_core.h compiled with g++ and the device math of
bh_math.h, with the search that supplies the phase velocities.  It includes the phase twin, so one library gives both
and `phase` below is sensitivity_cases.Twin on the same build.

SEDIMENT: sensitivity_cases.MODELS has no (model, period) with E < 0 -- the motion is retrograde at all thirty -- so the
checks of `absolute` get a strong-contrast model of their own: 400 m of soft sediment (vs 0.4 km/s) on rock.  Between
the periods at which the horizontal and the vertical surface motion vanish (about 0.9 T0 .. 2 T0 of the layer's
resonance T0 = 4 h / vs = 4 s) the fundamental mode is prograde, E < 0.  SEDIMENT_PERIODS has periods inside and on
either side of that window; test_ell_sens checks that both signs occur.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import sensitivity_cases as sc

SIM_SRCS = [os.path.join(sc.HOSTSIM, 'ell_sens_sim.cpp')] \
    + [os.path.join(sc.ROOT, 'bayhunter_amd', 'csrc', h) for h in ('ell_sens_core.h', 'ell_core.h')] + sc.SIM_SRCS
SIM_FLAGS = ['-O2', '-std=c++17', '-ffp-contract=off'] + sc.FMA
FORMS = {'tz': 0, 'tr': 1}

SEDIMENT = (np.array([0.4, 0.]), np.array([1.8, 5.2]), np.array([0.4, 3.0]), np.array([1.9, 2.6]))
SEDIMENT_PERIODS = np.array([1.5, 3.0, 5.0, 6.5, 12.0])


def load_sim():
    so = os.path.join(sc.HOSTSIM, 'libell_sens_sim.so')
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SIM_SRCS):
        subprocess.run(['g++'] + SIM_FLAGS + ['-fPIC', '-shared', '-o', so, SIM_SRCS[0]], check=True)
    lib = C.CDLL(so)
    vp, dp, i = C.c_void_p, C.POINTER(C.c_double), C.c_int
    lib.ss_sens_row.restype = None
    lib.ss_sens_row.argtypes = [dp, dp, dp, dp, i, i, i, i, dp, dp, i, dp, dp, dp, dp]
    lib.ss_sensitivity.restype = i
    lib.ss_sensitivity.argtypes = [vp, vp, vp, vp, i, i, i, dp, dp, dp, dp, dp]
    lib.es_ell_row.restype = None
    lib.es_ell_row.argtypes = [dp, dp, dp, dp, i, i, i, dp, dp, i, dp, i, i, i] + [dp] * 6
    lib.es_ell_sensitivity.restype = i
    lib.es_ell_sensitivity.argtypes = [vp, vp, vp, vp, i, i, dp, dp, i, i, i] + [dp] * 7
    lib.es_ell_value.restype = None
    lib.es_ell_value.argtypes = [dp, dp, dp, dp, i, i, dp, dp, i, dp]
    return EllTwin(lib)


def _steps(steps):
    if steps is None:
        return None, None
    st = np.ascontiguousarray(steps, dtype=np.float64)
    return st, st.ctypes.data_as(C.POINTER(C.c_double))


class EllTwin(object):
    def __init__(self, lib):
        self.lib = lib
        self.phase = sc.Twin(lib)

    def sensitivity(self, h, vp, vs, rho, periods, form='tz', absolute=False, total=True, steps=None):
        """es_ell_sensitivity: dict K, K_phase [nper][4][n], E, dE_dT, c, G_c, c0 (the search's phase velocities), err;
        layers real*4.  form: 'tz' (the kernels') or 'tr'; total False: K without the G_c dc/dm term; steps: the five
        relative steps (c, T, h, velocities, density) or None for the library's."""
        f = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)) for x in (h, vp, vs, rho)]
        t = np.ascontiguousarray(periods, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        n = len(f[0])
        K, Kp = np.zeros((t.size, 4, n)), np.zeros((t.size, 4, n))
        E, dE, c, g, cg = (np.zeros(t.size) for _ in range(5))
        keep, st = _steps(steps)
        err = self.lib.es_ell_sensitivity(*[x.ctypes.data for x in f], n, t.size, t.ctypes.data_as(dp), st, FORMS[form],
                                          int(bool(absolute)), int(bool(total)),
                                          *[x.ctypes.data_as(dp) for x in (K, E, dE, c, Kp, g, cg)])
        return dict(K=K, K_phase=Kp, E=E, dE_dT=dE, c=c, G_c=g, c0=cg, err=err)

    def row(self, h, vp, vs, rho, periods, c, nlay=None, Lmax=None, err=0, form='tz', absolute=False, total=True, steps=None,
            k_phase=True):
        """es_ell_row: one row of bh_ell_sens_batch from fp64 layers (nlay of them valid) and the phase velocities c:
        (K [nper][4][Lmax], E, dE_dT, c_out, K_phase)."""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (h, vp, vs, rho)]
        t, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (periods, c))
        nlay = len(a[0]) if nlay is None else int(nlay)
        Lmax = nlay if Lmax is None else int(Lmax)
        assert all(x.size >= min(max(nlay, 1), Lmax) for x in a)
        K, Kp = np.zeros((t.size, 4, Lmax)), np.zeros((t.size, 4, Lmax))
        E, dE, co = np.zeros(t.size), np.zeros(t.size), np.zeros(t.size)
        keep, st = _steps(steps)
        self.lib.es_ell_row(*[x.ctypes.data_as(dp) for x in a], nlay, Lmax, t.size, t.ctypes.data_as(dp), c.ctypes.data_as(dp),
                            int(err), st, FORMS[form], int(bool(absolute)), int(bool(total)),
                            *[x.ctypes.data_as(dp) for x in (K, E, dE, co)], Kp.ctypes.data_as(dp) if k_phase else None, None)
        return K, E, dE, co, Kp

    def value(self, h, vp, vs, rho, periods, c, absolute=False):
        """es_ell_value: ell_core.h's ell_value at the phase velocities c (what ell_kernel returns), layers real*4."""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)) for x in (h, vp, vs, rho)]
        t, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (periods, c))
        out = np.zeros(t.size)
        self.lib.es_ell_value(*[x.ctypes.data_as(dp) for x in a], len(a[0]), t.size, t.ctypes.data_as(dp), c.ctypes.data_as(dp),
                              int(bool(absolute)), out.ctypes.data_as(dp))
        return out
