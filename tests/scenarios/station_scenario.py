"""Shared by the station-pool tests (tests/test_stations.py, tests/test_gpu_stations.py) and tools/station_bench.py:
stations made from the tutorial's observed data -- station 0 is the tutorial station itself, the others have `y`
perturbed by a seeded draw and, when `yerr` is asked for, every station its own errors on the dispersion targets."""
import numpy as np

from chain_scenario import TWO, joint_target


def make_stations(data_dir, nstations, refs=TWO, oracle=None, yerr=False, seed=2024):
    """-> list of JointTargets.  yerr: the dispersion targets carry observational errors (a different draw per
    station), which selects the yerr-scaled covariance model when their noise correlation is fixed at 0."""
    out = []
    for s in range(nstations):
        joint = joint_target(data_dir, refs=refs, oracle=oracle)
        rng = np.random.RandomState(seed + s)
        for t in joint.targets:
            n = t.obsdata.y.size
            if s > 0:
                amp = 0.02 if t.noiseref == 'swd' else 0.005
                t.obsdata.y = t.obsdata.y + amp * rng.standard_normal(n)
            if yerr and t.noiseref == 'swd':
                t.obsdata.yerr = 0.01 + 0.03 * rng.uniform(size=n)
        out.append(joint)
    return out


def station_evaluator(evaluators):
    """One (packed, nlay, noise) -> (logL, misfits) function per station -> the four-argument function a
    StationPool takes: every row goes to the evaluator of its station."""
    def run(packed, nlay, noise, station):
        B = packed.shape[0]
        logL, misfits = np.zeros(B), None
        for s in np.unique(station):
            sel = np.nonzero(station == s)[0]
            l, m = evaluators[int(s)](packed[sel], nlay[sel], noise[sel])
            if misfits is None:
                misfits = np.zeros((B, np.asarray(m).shape[1]))
            logL[sel], misfits[sel] = l, m
        if misfits is None:
            misfits = np.zeros((0, 1))
        return logL, misfits
    return run
