"""Station pools made, run and closed back to back in ONE process (GPU box), in the style of pool_lifecycle.py:
every pool owns two evaluation plans with their observation tables on the device; a closed pool keeps its results
and refuses to run; every pool reproduces the first one's chains.

Prints one JSON line.  usage: station_lifecycle.py [npools] [nstations] [chains_per_station] [iterations]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(npools=5, nstations=48, c=8, iterations=40):
    from bayhunter_amd import _lib
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    data = os.path.join(ROOT, 'tests', 'golden', 'tutorial_observed')
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=iterations - 10, iter_main=10, acceptance=(40, 100))
    rs = list(range(nstations))
    rec = dict(pools=0, plans_closed=0, same_chains=0)

    def make():
        return StationPool(make_stations(data, nstations, yerr=True), ip, case['priors'], chains_per_station=c,
                           random_seeds=rs, groups=2)
    unrun = make()
    unrun.close()
    try:
        unrun.run()
        raise AssertionError('a closed pool ran')
    except _lib.BayHunterAmdError:
        pass
    first = None
    for k in range(npools):
        if k % 2 == 0:
            with make() as pool:
                pool.run()
                plans = list(pool.evaluator._plans.values())
                assert len(plans) == 2 and not any(p.closed for p in plans)
        else:
            pool = make()
            pool.run()
            plans = list(pool.evaluator._plans.values())
            pool.close()
            pool.close()
        assert pool.closed and all(p.closed for p in plans) and not pool.evaluator._plans
        rec['plans_closed'] += len(plans)
        got = {k2: pool.station(nstations - 1).chain(c - 1)[k2].copy() for k2 in ('models', 'likes', 'iter')}
        if first is None:
            first = got
        rec['same_chains'] += int(all(np.array_equal(first[k2], got[k2], equal_nan=True) for k2 in got))
        rec['pools'] += 1
    rec['ok'] = True
    print(json.dumps(rec))


if __name__ == '__main__':
    main(*[int(a) for a in sys.argv[1:]])
