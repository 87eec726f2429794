"""GPU tier: swd_kernel with its period table and the layer step's exact fusions (swd_core.h) returns the bits it
returned before, on the lane kernel in one pass, on the lane kernel with lanes pulling several searches from the work
queue, and on the 16-lane teams (which take the fusions, not the table).

Shapes, the smallest at which these paths can go wrong:
  ten       256 ten-layer models: four waves
  ragged    128 models of 2 .. 31 layers
  hunted    the models of tests/test_gpu_control_paths.py (every path of the control code; low-velocity zones)
  grid      the models of tests/test_gpu_recip_reuse.py whose scan meets a layer's vs or vp exactly (wvno == xkb, == xka)
  straddle  one wave of 64 models that differ in the vs of layer 2 alone, spread over 2.0 .. 3.2 km/s: whenever the trial
            velocity lies in that span, the lanes below it take the sincos arm of swd_var for that layer and the lanes
            above it the exp arm, in the same loop trip
Rayleigh and Love, phase and group velocity, 21 periods.

References.  Every value and flag must equal the host replay of the same sources with the device's math
(tests/hostsim/exact_rewrites_sim.cpp, reading the period table like swd_kernel).  The oracle port computes with glibc's
sin / cos / exp; the device's differ from those in the last bit of some values, which models whose velocity increases
with depth do not notice (tests/tolerances.py): on ten, ragged, grid and straddle -- all monotone -- every value and flag
must equal the oracle's too.  The hunted models have low-velocity zones: there the flags must equal the oracle's, and
the replay with glibc math equals the oracle bit for bit in tests/test_swd_exact_rewrites.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bayhunter_amd.synthetic import draw_models
from conftest import REFS, ROOT

PER = np.linspace(1, 41, 21)
MONOTONE = ('ten', 'ragged', 'grid', 'straddle')


def _straddle():
    import test_gpu_recip_reuse as R
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    h, vp, vs = (f32(x) for x in R._base(1.0))
    B = 64
    H, VP, VS = np.tile(h, (B, 1)), np.tile(vp, (B, 1)), np.tile(vs, (B, 1))
    VS[:, 2] = f32(np.linspace(2.0, 3.2, B))
    VP[:, 2] = f32(1.75 * VS[:, 2])
    assert np.all(np.diff(VS, axis=1) > 0) and np.all(np.diff(VP, axis=1) > 0)
    RHO = f32(VP * 0.32 + 0.77)
    return H, VP, VS, RHO, np.full(B, H.shape[1], dtype=np.int32)


def _ragged():
    """128 of 1 024 drawn models: the first of 2 and the first of 31 layers, and the 126 drawn first of the others."""
    m = draw_models(1024, (2, 31), seed=77002, sorted_vs=True)
    nl = m[4]
    ends = [int(np.flatnonzero(nl == 2)[0]), int(np.flatnonzero(nl == 31)[0])]
    idx = sorted(ends + [i for i in range(len(nl)) if i not in ends][:126])
    return tuple(np.ascontiguousarray(a[idx]) for a in m)


def shapes():
    import test_gpu_control_paths as T
    import test_gpu_recip_reuse as R
    g = R._constructed()
    return {
        'ten': draw_models(256, 10, seed=77001, sorted_vs=True),
        'ragged': _ragged(),
        'hunted': tuple(T.batch()),
        'grid': (g[0], g[1], g[2], g[3], np.full(g[0].shape[0], g[0].shape[1], dtype=np.int32)),
        'straddle': _straddle(),
    }


def engine_run(models):
    from bayhunter_amd.engine import ForwardEngine, SwdSpec
    eng = ForwardEngine(swd=[SwdSpec(r[0], PER) for r in REFS])
    out, err = eng.run(*models)
    out, err = out.cpu().numpy(), err.cpu().numpy()
    return [out[:, eng.slices[t]] for t in range(len(REFS))], err


@pytest.fixture(scope='module')
def refs(oracle):
    """{shape: (models, [per target: replay values, replay err, oracle values, oracle err])}, computed once."""
    from test_swd_exact_rewrites import build_sim, replay_batch
    sim = build_sim()
    res = {}
    for name, models in shapes().items():
        per_target = []
        for _, iwave, igr in REFS:
            cg, err = replay_batch(sim, models, PER, iwave, igr)
            want, werr, _ = oracle.swd_batch(*models, PER, iwave, igr, nthreads=8)
            per_target.append((cg, err, want, werr))
        res[name] = (models, per_target)
    return res


def _compare(vals, err, per_target, shape, form):
    for t, (cg, rerr, want, werr) in enumerate(per_target):
        where = (shape, form, REFS[t][0])
        assert np.array_equal(err[:, t], rerr) and np.array_equal(err[:, t], werr), where
        assert np.array_equal(vals[t].view(np.int64), cg.view(np.int64)), where + (int((vals[t] != cg).sum()),)
        if shape in MONOTONE:
            assert np.array_equal(vals[t].view(np.int64), want.view(np.int64)), where + (int((vals[t] != want).sum()),)


def test_shapes_and_references(refs):
    """CPU part: the shapes are what the header says, the straddle wave does straddle, and the monotone shapes' replay
    already equals the oracle."""
    assert {k: len(v[0][4]) for k, v in refs.items()} == {'ten': 256, 'ragged': 128, 'hunted': 217, 'grid': 8, 'straddle': 64}
    nl = refs['ragged'][0][4]
    assert nl.min() == 2 and nl.max() == 31
    vs2 = refs['straddle'][0][2][:, 2]
    c = refs['straddle'][1][0][2]                                   # Rayleigh phase velocities of the oracle
    inside = (c > vs2.min()) & (c < vs2.max())                      # roots between the wave's smallest and largest vs2
    assert inside.any(axis=1).all(), 'every lane must have a root inside the span of layer 2'
    for name in MONOTONE:
        for t, (cg, rerr, want, werr) in enumerate(refs[name][1]):
            assert np.array_equal(rerr, werr) and np.array_equal(cg.view(np.int64), want.view(np.int64)), (name, t)
    for t, (cg, rerr, want, werr) in enumerate(refs['hunted'][1]):
        print('hunted, %s: %d of %d values of the device-math replay are not the oracle\'s' % (REFS[t][0], (cg != want).sum(), cg.size))
        assert np.array_equal(rerr, werr), t


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['lane', 'team16'])
@pytest.mark.parametrize('shape', ['ten', 'ragged', 'hunted', 'grid', 'straddle'])
def test_gpu_forms_return_the_replay_and_the_oracle(lib, refs, shape, form):
    from bayhunter_amd import _lib
    models, per_target = refs[shape]
    _lib.set_swd_kernel(form)
    try:
        vals, err = engine_run(models)
    finally:
        _lib.set_swd_kernel('auto')
    _compare(vals, err, per_target, shape, form)


@pytest.mark.gpu
def test_gpu_queue_form_returns_the_replay_and_the_oracle(lib, refs, tmp_path):
    """One resident wave per target (test hook BH_SWD_RESIDENT_WAVES, read once per process: hence the child, one for
    all shapes): every lane pulls several searches from the work queue beside lanes in other states."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_exact_rewrites as T
from bayhunter_amd import _lib
_lib.set_swd_kernel('lane')
res = {}
for name, models in T.shapes().items():
    vals, err = T.engine_run(models)
    res[name + '_err'] = err
    for t, v in enumerate(vals):
        res['%%s_v%%d' %% (name, t)] = v
np.savez(sys.argv[1], **res)
""" % (ROOT, os.path.join(ROOT, 'tests'))
    path = str(tmp_path / 'queue.npz')
    subprocess.run([sys.executable, '-c', code, path], check=True, env=dict(os.environ, BH_SWD_RESIDENT_WAVES='3'))
    got = np.load(path)
    for shape, (_, per_target) in refs.items():
        _compare([got['%s_v%d' % (shape, t)] for t in range(len(REFS))], got[shape + '_err'], per_target, shape, 'queue')
