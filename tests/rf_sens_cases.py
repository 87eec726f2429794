"""Shared by tests/test_rf_sens.py, tests/test_gpu_rf_sens.py and tests/rf_sens_tolerances.py: the host twin of
rf_sens_kernel (tests/hostsim/rf_sens_sim.cpp: bayhunter_amd/csrc/rf_sens_core.h compiled with g++ and the device math
of bh_math.h) and the case lists.

MODELS (the list the steps were tuned on; each for 'prf' and 'srf' at nsamp 128 and 256: CASES):
    L1        a half-space alone.  Nothing is transmitted upward into a half-space from below: the spectral division is
              0 / 0 and the trace NaN, in the reference as in bh_rf_batch.  K is NaN with it (but the 0 of K_h); the
              case checks exactly that and takes no part in the sweep
    L2        one layer over a half-space
    L3        two layers over a half-space
    sediment  0.6 km of slow sediment on a crust of three layers
    lvz       five layers with a low-velocity zone in the middle crust
    L12       twelve layers, velocity increasing with depth
OFFLIST: models nothing was tuned on (draws of bayhunter_amd.synthetic.draw_models, other slowness and Gauss factor).

The reference (tests/rf_sens_ref.py) flags entries where the trace is not differentiable; reference_flags() counts them per
list, and test_rf_sens.py holds both lists to rf_sens_ref.CAP (measured when the lists were fixed: none flagged).
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, 'tests', 'hostsim')
SIM_SRCS = [os.path.join(HOSTSIM, 'rf_sens_sim.cpp')] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', h) for h in
                                                         ('rf_sens_core.h', 'rf_core.h', 'rf_host.h', 'sens_core.h',
                                                          'swd_core.h', 'bh_math.h', 'bh_common.h')]
FMA = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
SIM_FLAGS = ['-O2', '-std=c++17', '-ffp-contract=off'] + FMA
KINDS = ('h', 'vp', 'vs', 'rho')


def _model(vs, h, vpvs=1.75):
    vs, h = np.array(vs, dtype=np.float64), np.array(h, dtype=np.float64)
    vp = vpvs * vs
    return h, vp, vs, 0.77 + 0.32 * vp


MODELS = {
    'L1': _model([3.5], [0.]),
    'L2': _model([3.4, 4.4], [30., 0.]),
    'L3': _model([2.9, 3.7, 4.5], [6., 26., 0.]),
    'sediment': _model([1.4, 3.2, 3.6, 3.9, 4.5], [0.6, 9., 12., 14., 0.]),
    'lvz': _model([3.0, 3.5, 3.1, 3.8, 4.0, 4.5], [4., 8., 6., 9., 11., 0.]),
    'L12': _model(np.linspace(2.4, 4.6, 12), [1.5, 2., 2.5, 3., 3., 4., 4., 5., 5., 6., 6., 0.]),
}


def params(ref='prf', nsamp=256, p=6.4, gauss=1.0, fsamp=5.0, tshift=5.0, nsv=None, nout=None):
    return dict(p=p, gauss=gauss, nsamp=nsamp, fsamp=fsamp, tshift=tshift, nsv=nsv, waveno=1 if ref == 'srf' else 0,
                nout=nsamp if nout is None else nout)


CASES = [(name, ref, nsamp) for name in MODELS for ref in ('prf', 'srf') for nsamp in (128, 256)]


def _drawn(seed, n):
    from bayhunter_amd.synthetic import draw_models
    H, VP, VS, RHO, nl = draw_models(1, n, seed=seed)
    return H[0, :n].copy(), VP[0, :n].copy(), VS[0, :n].copy(), RHO[0, :n].copy()


OFFLIST = {
    'draw4': (_drawn(301, 4), params('prf', 256, p=5.1, gauss=1.6)),
    'draw7': (_drawn(302, 7), params('srf', 128, p=7.3, gauss=0.9)),
    'draw9': (_drawn(303, 9), params('prf', 128, p=4.4, gauss=2.0, nsv=3.1)),
}


def load_sim():
    so = os.path.join(HOSTSIM, 'librf_sens_sim.so')
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SIM_SRCS):
        subprocess.run(['g++'] + SIM_FLAGS + ['-fPIC', '-shared', '-o', so, SIM_SRCS[0]], check=True)
    lib = C.CDLL(so)
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    lib.rs_rf_sens_row.restype = None
    lib.rs_rf_sens_row.argtypes = [i, i, vp, vp, vp, vp, vp, vp, d, d, i, d, d, d, d, i, i, vp, vp, vp]
    lib.rs_steps.restype = None
    lib.rs_steps.argtypes = [vp]
    lib.rs_slot.restype = lib.rs_pairs.restype = i
    lib.rs_pairs.argtypes = [i, i]
    lib.rs_lds_bytes.restype = C.c_long
    lib.rs_lds_bytes.argtypes = [i, i]
    lib.rs_slot.argtypes = [i, i]
    return Twin(lib)


class Twin(object):
    def __init__(self, lib):
        self.lib = lib

    def steps(self):
        s = np.zeros(4)
        self.lib.rs_steps(s.ctypes.data)
        return s

    def row(self, h, vp, vs, rho, par, nlay=None, Lmax=None, steps=None, qp=None, qs=None, sigma=np.nan):
        """rs_rf_sens_row: one row of bh_rf_sens_batch, (K [nout][4][Lmax], rf [nout]).  The rows may be longer than nlay
        (padding is never read); steps: (h, vp, vs, rho) or None for the library's."""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (h, vp, vs, rho)]
        nlay = len(a[0]) if nlay is None else int(nlay)
        Lmax = nlay if Lmax is None else int(Lmax)
        a = [np.concatenate([x, np.full(max(0, Lmax - x.size), 7.7)]) for x in a]
        q = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (qp, qs)]
        st = None if steps is None else np.ascontiguousarray(steps, dtype=np.float64)
        K, rf = np.zeros((par['nout'], 4, Lmax)), np.zeros(par['nout'])
        self.lib.rs_rf_sens_row(nlay, Lmax, *[x.ctypes.data for x in a], *[None if x is None else x.ctypes.data for x in q],
                                par['p'], par['gauss'], par['nsamp'], par['fsamp'], par['tshift'],
                                -1.0 if par['nsv'] is None else par['nsv'], sigma, par['waveno'], par['nout'],
                                None if st is None else st.ctypes.data, K.ctypes.data, rf.ctypes.data)
        return K, rf


_REF = {}


def _ref_task(task):
    import rf_sens_ref
    model, par = task
    return rf_sens_ref.kernels(*model, par)


def references(keys):
    """{key: rf_sens_ref.kernels(...)} for keys of CASES (name, ref, nsamp) or names of OFFLIST, computed once per
    session in a few processes and not changed."""
    import multiprocessing as mp
    todo = [k for k in keys if k not in _REF]
    if todo:
        tasks = [OFFLIST[k] if k in OFFLIST else (MODELS[k[0]], params(k[1], k[2])) for k in todo]
        with mp.get_context('fork').Pool(min(8, os.cpu_count() or 1)) as pool:
            for k, r in zip(todo, pool.map(_ref_task, tasks, chunksize=1)):
                _REF[k] = r
    return {k: _REF[k] for k in keys}


def reference_flags(keys):
    """(flagged entries, all (model, sample, slot) entries) of a list"""
    refs = references(keys)
    flagged = sum(int(r['flagged'].sum()) for r in refs.values())
    total = sum(r['K'].shape[0] * (4 * r['K'].shape[2] - 1) for r in refs.values())
    return flagged, total
