"""The host twin of the group-velocity sensitivity kernels, shared by tests/test_sens_group.py, tests/test_gpu_sens_group.py
and tests/sens_group_tolerances.py.  Models, periods and the rows without a value are sensitivity_cases'.

The twin is tests/hostsim/sens_group_sim.cpp: bayhunter_amd/csrc/sens_group_core.h compiled with g++ and the device math
of bh_math.h, with the search that supplies the phase velocities.  It includes the phase twin, so one library gives
both and `phase` below is sensitivity_cases.Twin on the same build.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import sensitivity_cases as sc

SIM_SRCS = [os.path.join(sc.HOSTSIM, 'sens_group_sim.cpp'), os.path.join(sc.ROOT, 'bayhunter_amd', 'csrc', 'sens_group_core.h')] \
    + sc.SIM_SRCS
SIM_FLAGS = ['-O2', '-std=c++17', '-ffp-contract=off'] + sc.FMA


def load_sim():
    so = os.path.join(sc.HOSTSIM, 'libsens_group_sim.so')
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SIM_SRCS):
        subprocess.run(['g++'] + SIM_FLAGS + ['-fPIC', '-shared', '-o', so, SIM_SRCS[0]], check=True)
    lib = C.CDLL(so)
    vp, dp, d = C.c_void_p, C.POINTER(C.c_double), C.c_double
    lib.ss_sens_row.restype = None
    lib.ss_sens_row.argtypes = [dp, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, dp, dp, dp, dp]
    lib.ss_sensitivity.restype = C.c_int
    lib.ss_sensitivity.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp]
    lib.sg_group_row.restype = None
    lib.sg_group_row.argtypes = [dp, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, dp, d, d] + [dp] * 6
    lib.sg_group_sensitivity.restype = C.c_int
    lib.sg_group_sensitivity.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, dp, d, d] + [dp] * 7
    return GroupTwin(lib)


class GroupTwin(object):
    def __init__(self, lib):
        self.lib = lib
        self.phase = sc.Twin(lib)

    def sensitivity(self, h, vp, vs, rho, periods, wave='rayleigh', rg=0.0, window=-1.0):
        """sg_group_sensitivity: dict K, K_phase [nper][4][n], U, dU_dT, c, dc_dT, c0 (the search's phase velocities), err;
        layers real*4.  rg: the step over T (0: the library's); window: the side roots' (negative: the step's own)."""
        f = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)) for x in (h, vp, vs, rho)]
        t = np.ascontiguousarray(periods, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        n = len(f[0])
        K, Kp = np.zeros((t.size, 4, n)), np.zeros((t.size, 4, n))
        U, dU, c, d, cg = (np.zeros(t.size) for _ in range(5))
        err = self.lib.sg_group_sensitivity(*[x.ctypes.data for x in f], n, sc.WAVES[wave], t.size, t.ctypes.data_as(dp),
                                            float(rg), float(window), *[x.ctypes.data_as(dp) for x in (K, U, dU, c, Kp, d, cg)])
        return dict(K=K, K_phase=Kp, U=U, dU_dT=dU, c=c, dc_dT=d, c0=cg, err=err)

    def row(self, h, vp, vs, rho, periods, c, wave='rayleigh', nlay=None, Lmax=None, err=0, rg=0.0, window=-1.0):
        """sg_group_row: one row of bh_sens_group_batch from fp64 layers (nlay of them valid) and the phase velocities c:
        (K [nper][4][Lmax], U, dU_dT, c_out, K_phase)."""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (h, vp, vs, rho)]
        t, c = (np.ascontiguousarray(x, dtype=np.float64) for x in (periods, c))
        nlay = len(a[0]) if nlay is None else int(nlay)
        Lmax = nlay if Lmax is None else int(Lmax)
        assert all(x.size >= min(max(nlay, 1), Lmax) for x in a)
        K, Kp = np.zeros((t.size, 4, Lmax)), np.zeros((t.size, 4, Lmax))
        U, dU, co = np.zeros(t.size), np.zeros(t.size), np.zeros(t.size)
        self.lib.sg_group_row(*[x.ctypes.data_as(dp) for x in a], nlay, Lmax, sc.WAVES[wave], t.size, t.ctypes.data_as(dp),
                              c.ctypes.data_as(dp), int(err), None, float(rg), float(window),
                              *[x.ctypes.data_as(dp) for x in (K, U, dU, co, Kp)], None)
        return K, U, dU, co, Kp
