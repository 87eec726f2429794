"""Shared by test_rf_floor.py (CPU tier) and test_gpu_rf_floor.py (GPU tier): the host replay of rf_kernel with the
bounded attenuation exponent and the radix-4 passes (tests/hostsim/rf_floor_sim.cpp -> rf_host.h: rf_host_replay), and
the models on which the two forms of the exponential meet inside one wave."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SIM = {}


def floor_sim():
    """g++ build of rf_floor_sim.cpp with the device math of bh_math.h (conftest: hostsim_devmath's flags)."""
    if 'hs' in _SIM:
        return _SIM['hs']
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so, src = os.path.join(d, 'librf_floor_sim.so'), os.path.join(d, 'rf_floor_sim.cpp')
    deps = [src] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', f) for f in ('bh_common.h', 'bh_math.h', 'rf_core.h', 'rf_host.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        fma = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + fma + ['-o', so, src], check=True)
    hs = C.CDLL(so)
    vp_, i_, d_ = C.c_void_p, C.c_int, C.c_double
    hs.hs_rf_floor.restype = None
    hs.hs_rf_floor.argtypes = [i_, vp_, vp_, vp_, vp_, vp_, vp_, d_, d_, i_, d_, d_, d_, i_, i_, vp_, i_]
    hs.hs_exp_forms.restype = d_
    hs.hs_exp_forms.argtypes = [i_, vp_, vp_, vp_]
    hs.hs_cexp_pair.restype = hs.hs_cexp_full.restype = None
    hs.hs_cexp_pair.argtypes = [i_, vp_, vp_, vp_]
    hs.hs_cexp_full.argtypes = [i_, vp_, vp_]
    _SIM['hs'] = hs
    return hs


def replay(h, vp, vs, rho, p=6.4, gauss=1.0, nsamp=512, fsamp=5.0, tshift=5.0, nsv=None, waveno=0, nout=201, qp=None,
           qs=None, radix4=True):
    """One model through rf_host_replay; the arguments of conftest's HS.rf."""
    hs = floor_sim()
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (h, vp, vs, rho)]
    q = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (qp, qs)]
    out = np.zeros(nout)
    hs.hs_rf_floor(len(a[0]), *[x.ctypes.data for x in a], *[None if x is None else x.ctypes.data for x in q], p, gauss,
                   nsamp, fsamp, tshift, -1.0 if nsv is None else nsv, waveno, nout, out.ctypes.data, 1 if radix4 else 0)
    return out


GAUSS_ALL = 1.3          # a >= 1.21: no Gauss cut-off, all 257 frequencies of 512 samples at 5 Hz: w up to 15.7 rad/s


def mixed_bound_models(count, seed=11):
    """Q_s = 5 (Q_p = 10) over a thick slow layer under a thin one: the attenuation exponent w d Im(slowness), about
    w d / (2 Q v), passes the kernel's bound (0.34) between the first and the ninth frequency and reaches 4 ... 9 at
    w = 15.7 rad/s, so the model's first wave of phase 3 holds arguments on both sides of the bound and its other waves
    only arguments outside it."""
    rs = np.random.RandomState(seed)
    for _ in range(count):
        n = rs.randint(3, 7)
        h = np.concatenate((rs.uniform(0.5, 2.0, 1), rs.uniform(10.0, 15.0, 1), rs.uniform(2.0, 8.0, n - 3), [0.]))
        vs = np.concatenate(([rs.uniform(2.0, 2.4)], [rs.uniform(2.5, 2.8)], np.sort(rs.uniform(3.0, 4.8, n - 2))))
        vp = vs * rs.uniform(1.7, 1.9)
        yield dict(h=h, vp=vp, vs=vs, rho=0.77 + 0.32 * vp, qp=np.full(n, 10.0), qs=np.full(n, 5.0),
                   z=np.concatenate(([0], np.cumsum(h)[:-1])), gauss=GAUSS_ALL, p=float(rs.uniform(4, 8)), waveno=0,
                   sigma=float((2 - (vp[0] / vs[0]) ** 2) / (2 - 2 * (vp[0] / vs[0]) ** 2)))


def attenuation_exponents(m, nsamp=512, fsamp=5.0):
    """[nfreq][nlay - 1][2]: the real parts of the two exponentials' arguments of every (frequency, layer) step of
    phase 3 for model m, from the formulas of rf_phase3_body on the unflattened model (earth flattening moves them by
    a fraction of a per cent)."""
    w = 2.0 * np.pi * fsamp / nsamp * np.arange(nsamp // 2 + 1)
    lgw = np.where(w > 0, np.log(np.maximum(w, 1e-300) / (2.0 * np.pi)), 0.0)[:, None]
    u2 = (m['p'] * 0.00899) ** 2
    out = []
    for v, q in ((m['vp'], m['qp']), (m['vs'], m['qs'])):
        a = 1.0 / (np.pi * q[None, :-1])
        f = 1.0 + lgw * a + 1j * a * (0.5 * np.pi)
        out.append(w[:, None] * m['h'][None, :-1] * np.sqrt(1.0 / (f * f) / v[None, :-1] ** 2 - u2).imag)
    return np.stack(out, axis=-1)
