"""Every path of the throughput kernel's control code and event pass, bit for bit against the host replay.

swd_control / swd_neville for a table in registers are written as flags and selects, and swd_lane takes its events
in one straight pass.  The bench workloads walk through the common paths only, so this batch
is hunted: 217 ragged models (2 .. 31 layers; not a multiple of 64, so lanes of a wave are in different states and the
last wave is partly empty) -- the first 48 draws of four seeds, the models of those seeds that the replay's counters
single out, and the 13 models of the LVZ worst-case fixture -- under three targets:

    T0  Rayleigh phase, 2 modes, 21 periods 1 .. 41 s
    T1  Rayleigh group, 2 modes, the same periods        (second solve of a group-velocity pair)
    T2  Rayleigh phase, 3 modes, 9 periods 20 .. 60 s    (modes cut off at their first period: an event stays pending
                                                          after the pass and the lane sits out a trip)

The models were found with tests/hostsim/control_paths_sim.cpp over draw_models(1000, (2, 31), seed, sorted_vs=False)
of seeds 70000 .. 70015; only seeds and indices are kept.  A table of 10 points (and one of 11, the longest there is)
turned up within 16 000 draws, so nothing is waived.

CPU tier: the replay -- the loop of swd_lane with the device's math -- counts the paths, and beside the flat control
code it runs the generic one (table in memory) on a copy of the state; both must leave the same state and table after
every evaluation.  Each path below must be hit.  GPU tier: the lane kernel in one pass, the lane kernel with lanes
pulling several searches from the work queue, and the 16-lane teams return the replay's values and error flags, every
bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bayhunter_amd.synthetic import draw_models
from conftest import ROOT

LMAX = 31
ORDINARY = range(48)
HUNTED = {
    70004: [102, 225, 373, 514, 786],
    70006: [52, 53, 157, 264, 540, 852],
    70010: [214],
    70014: [],
}
PER_A, PER_B = np.linspace(1, 41, 21), np.linspace(20, 60, 9)
TARGETS = [('rdispph', 2, 0, 2, PER_A), ('rdispgr', 2, 1, 2, PER_A), ('rdispph', 2, 0, 3, PER_B)]   # name, iwave, igr, modes
# counters of control_paths_sim.cpp
POINTS0, GUARD, TURN, NOROOT1, NOROOT2, LEFTOVER, MODE2, EVALS, NCNT = 0, 12, 13, 14, 15, 16, 17, 18, 24


def batch():
    parts = []
    for seed in sorted(HUNTED):
        H, VP, VS, RHO, nl = draw_models(1000, (2, LMAX), seed=seed, sorted_vs=False)
        idx = sorted(set(ORDINARY) | set(HUNTED[seed]))
        parts.append([a[idx] for a in (H, VP, VS, RHO, nl)])
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'lvz_worst_cases.npz'))
    for i in range(int(z['ncases'])):                           # every model of the LVZ worst-case fixture
        nl = z['c%d_nl' % i]
        assert nl.max() <= LMAX
        lv = []
        for k in ('H', 'VP', 'VS', 'RHO'):
            a = np.zeros((len(nl), LMAX))
            src = z['c%d_%s' % (i, k)]
            a[:, :src.shape[1]] = src
            lv.append(a)
        parts.append(lv + [nl])
    # interleaved, so that every wave holds hunted, ordinary and LVZ models
    H, VP, VS, RHO, nl = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    order = np.random.RandomState(11).permutation(len(nl))
    return [np.ascontiguousarray(a[order]) for a in (H, VP, VS, RHO)] + [np.ascontiguousarray(nl[order], dtype=np.int32)]


@pytest.fixture(scope='module')
def replay():
    """(models, [per target: values, err, counters]) from the host replay with the device's math, computed once."""
    d = os.path.join(ROOT, 'tests', 'hostsim')
    so, src = os.path.join(d, 'libcontrol_paths_sim.so'), os.path.join(d, 'control_paths_sim.cpp')
    deps = [src] + [os.path.join(ROOT, 'bayhunter_amd', 'csrc', f) for f in ('bh_common.h', 'bh_math.h', 'swd_core.h')]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        fma = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off'] + fma + ['-o', so, src],
                       check=True)
    hs = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    hs.cp_batch.restype = C.c_int
    hs.cp_batch.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, ip] + [C.c_int] * 5 + [dp, dp, ip, C.POINTER(C.c_long)]
    models = batch()
    H, VP, VS, RHO, nl = models
    B = len(nl)
    res = []
    for _, iw, ig, mode, per in TARGETS:
        per = np.ascontiguousarray(per, dtype=np.float64)
        cg, err, cnt = np.zeros((B, len(per))), np.zeros(B, np.int32), np.zeros((B, NCNT), np.int64)
        rc = hs.cp_batch(B, LMAX, *[a.ctypes.data_as(dp) for a in (H, VP, VS, RHO)], nl.ctypes.data_as(ip), 0, iw, mode,
                         ig, len(per), per.ctypes.data_as(dp), cg.ctypes.data_as(dp), err.ctypes.data_as(ip),
                         cnt.ctypes.data_as(C.POINTER(C.c_long)))
        assert rc == 0, 'flat and generic control code part ways (target %s, %d modes): %d' % (TARGETS[len(res)][0], mode, rc)
        res.append((cg, err, cnt))
    return models, res


def test_batch_shape(replay):
    nl = replay[0][4]
    assert len(nl) == 217 and len(nl) % 64 != 0
    assert nl.min() == 2 and nl.max() == LMAX                   # ragged depths 2 .. 31
    assert len(np.unique(nl)) >= 25


def test_every_path_is_taken(replay):
    _, res = replay
    tot = [r[2].sum(0) for r in res]
    models = [(r[2] > 0).sum(0) for r in res]
    for t, (name, _, _, mode, _) in enumerate(TARGETS):
        print('%s, %d modes: evaluations %d, tables by points %s, guard %d, turn %d, no root 1st/2nd %d/%d, pending %d, '
              'higher-mode evaluations %d' % (name, mode, tot[t][EVALS], tot[t][2:12].tolist(), tot[t][GUARD],
                                              tot[t][TURN], tot[t][NOROOT1], tot[t][NOROOT2], tot[t][LEFTOVER], tot[t][MODE2]))
    for t in (0, 1):                                            # phase and group target alike
        for points in (2, 4, 7, 10):
            assert tot[t][POINTS0 + points] > 0, (t, points)
        assert tot[t][GUARD] > 0 and tot[t][TURN] > 0 and tot[t][NOROOT1] > 0 and tot[t][MODE2] > 0, t
        assert models[t][GUARD] >= 2 and models[t][TURN] >= 2, t
    assert tot[1][NOROOT2] > 0                                  # no root on the second solve of a group-velocity pair
    assert tot[2][LEFTOVER] > 0 and tot[2][NOROOT1] > 0         # an event left pending by the pass
    assert tot[0][NOROOT2] == 0 and tot[0][LEFTOVER] == 0       # (the counters tell the paths apart)


def test_replay_is_the_host_replay_of_the_suite(replay, hostsim_devmath):
    """The counting replay returns what the suite's own replay of swd_lane returns (a sample of the batch)."""
    (H, VP, VS, RHO, nl), res = replay
    for t, (_, iw, ig, mode, per) in enumerate(TARGETS):
        for b in range(0, len(nl), 9):
            n = nl[b]
            cg, e, _ = hostsim_devmath.swd(H[b, :n], VP[b, :n], VS[b, :n], RHO[b, :n], per, iw, ig, mode=mode)
            assert e == res[t][1][b] and np.array_equal(cg, res[t][0][b]), (t, b)


def _engine_run(models):
    from bayhunter_amd.engine import ForwardEngine, SwdSpec
    eng = ForwardEngine(swd=[SwdSpec(name, per, mode=mode) for name, _, _, mode, per in TARGETS])
    out, err = eng.run(*models)
    out, err = out.cpu().numpy(), err.cpu().numpy()
    return [out[:, eng.slices[t]] for t in range(len(TARGETS))], err


def _compare(vals, err, res, what):
    for t in range(len(TARGETS)):
        assert np.array_equal(err[:, t], res[t][1]), (what, t)
        assert np.array_equal(vals[t], res[t][0]), (what, t, int((vals[t] != res[t][0]).any(axis=1).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['lane', 'team16'])
def test_gpu_forms_return_the_replay(lib, replay, form):
    from bayhunter_amd import _lib
    models, res = replay
    _lib.set_swd_kernel(form)
    try:
        vals, err = _engine_run(models)
    finally:
        _lib.set_swd_kernel('auto')
    _compare(vals, err, res, form)


@pytest.mark.gpu
def test_gpu_queue_form_returns_the_replay(lib, replay, tmp_path):
    """One resident wave per target (test hook BH_SWD_RESIDENT_WAVES, read once per process: hence the child): every
    lane pulls three or four searches from the work queue, one after the other, beside lanes in other states."""
    models, res = replay
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_control_paths as T
from bayhunter_amd import _lib
_lib.set_swd_kernel('lane')
vals, err = T._engine_run(T.batch())
np.savez(sys.argv[1], err=err, **{'v%%d' %% t: v for t, v in enumerate(vals)})
""" % (ROOT, os.path.join(ROOT, 'tests'))
    path = str(tmp_path / 'queue.npz')
    subprocess.run([sys.executable, '-c', code, path], check=True, env=dict(os.environ, BH_SWD_RESIDENT_WAVES='3'))
    got = np.load(path)
    _compare([got['v%d' % t] for t in range(len(TARGETS))], got['err'], res, 'queue')
