"""GPU box: what putting many stations into one chain pool buys, on the tutorial inversion (Rayleigh phase + P-RF, free
vp/vs and noise, like tools/chain_bench.py).  For S stations of c chains each, three ways to run the S * c chains:

    stations   one StationPool of S x c chains, every station its own observed data
    onepool    one ChainPool of S * c chains on ONE station (the pool's speed when no observation sets are involved;
               with --root pointing at a checkout of another commit: that commit's pool, for before/after)
    singles    S single-station ChainPools of c chains, one after the other -- what is done without the feature.
               For S > --sample only --sample of them are timed and the time is scaled by S / --sample (said in
               the output: "scaled": true)

    python tools/station_bench.py [--modes stations,onepool,singles] [--repeats 5] [--sample 16] [--root DIR]
                                  [--vary-p LO HI] [--out FILE.jsonl] [SxC ...]   (default 64x16 256x16 1024x16 1024x4)

--vary-p LO HI: every station its own receiver-function ray parameter, spread evenly over [LO, HI] s/deg; the station
pool runs with per_station=('p',) (the per-row form of rf_kernel), the single pools each at their station's p, `onepool`
at station 0's.

A warm-up pool of every mode runs first; then `--repeats` rounds, each round running every mode once (alternating,
so that a drift of the box hits all modes alike).  One JSON line per (S, c, mode) with every repeat's seconds,
their median / min / max and chain iterations per second from the median; appended to --out if given."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('configs', nargs='*', default=['64x16', '256x16', '1024x16', '1024x4'])
    ap.add_argument('--modes', default='stations,onepool,singles')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sample', type=int, default=16)
    ap.add_argument('--iters', type=int, default=None, help='burn-in iterations (main phase: half of it)')
    ap.add_argument('--root', default=None, help='tree whose bayhunter_amd is measured (default: this one)')
    ap.add_argument('--vary-p', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                    help="stations with p spread evenly over [LO, HI] s/deg, pooled with per_station=('p',)")
    ap.add_argument('--tag', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = os.path.abspath(args.root) if args.root else here
    sys.path.insert(0, os.path.join(here, 'tests', 'scenarios'))
    sys.path.insert(0, root)
    from chain_scenario import CASES
    from station_scenario import make_stations
    import bayhunter_amd
    from bayhunter_amd.chains import ChainPool
    assert os.path.abspath(os.path.dirname(os.path.dirname(bayhunter_amd.__file__))) == root
    modes = args.modes.split(',')
    data = os.path.join(here, 'tests', 'golden', 'tutorial_observed')
    case = CASES['tutorial']

    def params(iters):
        return dict(case['initparams'], iter_burnin=iters, iter_main=iters // 2, acceptance=(40, 100))

    def seeds_of(S, c):        # station s: RandomState(s).randint(1000) per chain, in every mode
        out = []
        for s in range(S):
            rstate = np.random.RandomState(s)
            out.append([rstate.randint(1000) for _ in range(c)])
        return np.asarray(out)

    def run(mode, S, c, iters, stations):
        """-> (seconds of run(), stations actually run)"""
        ip, seeds = params(iters), seeds_of(S, c)
        kw = dict(nmodels=iters + iters // 2 + 1)     # room for every iteration
        if mode == 'stations':
            from bayhunter_amd.stations import StationPool
            per = dict(per_station=('p',)) if args.vary_p else {}
            with StationPool(stations, ip, case['priors'], seeds=seeds, **per, **kw) as pool:
                t0 = time.perf_counter()
                pool.run()
                return time.perf_counter() - t0, S
        if mode == 'onepool':
            with ChainPool(stations[0], ip, case['priors'], seeds=seeds.reshape(-1), **kw) as pool:
                t0 = time.perf_counter()
                pool.run()
                return time.perf_counter() - t0, S
        k = min(S, args.sample)
        dt = 0.0
        for s in range(k):                      # construction and close() of a pool are not counted: run() only
            with ChainPool(stations[s], ip, case['priors'], seeds=seeds[s], **kw) as pool:
                t0 = time.perf_counter()
                pool.run()
                dt += time.perf_counter() - t0
        return dt, k

    for cfg in args.configs:
        S, c = (int(v) for v in cfg.lower().split('x'))
        iters = args.iters or (120 if S * c <= 4096 else 60)
        stations = make_stations(data, S, yerr=True)
        if args.vary_p:
            for joint, p in zip(stations, np.linspace(args.vary_p[0], args.vary_p[1], S)):
                joint.targets[1].moddata.plugin.set_modelparams(p=float(p))
        for mode in modes:                      # first-use costs (kernel forms, helper threads, pinned buffers, the
            run(mode, S, c, 6, stations)        # set-up's factorisation) are not chain iterations
        time.sleep(0.25)                        # numpy's BLAS workers spin ~0.1 s after the set-up's factorisation
        secs = {m: [] for m in modes}
        ran = {}
        for _ in range(args.repeats):
            for mode in modes:
                dt, k = run(mode, S, c, iters, stations)
                secs[mode].append(dt * S / k)
                ran[mode] = k
        total = S * c * (iters + iters // 2)
        for mode in modes:
            v = np.asarray(secs[mode])
            rec = dict(bench='station_pool', tag=args.tag, vary_p=args.vary_p, mode=mode, stations=S, chains_per_station=c, chains=S * c,
                       iterations=iters + iters // 2, repeats=args.repeats, seconds=[round(float(x), 4) for x in v],
                       median_s=round(float(np.median(v)), 4), min_s=round(float(v.min()), 4),
                       max_s=round(float(v.max()), 4), chain_iterations_per_s=round(total / float(np.median(v))),
                       stations_timed=ran[mode], scaled=bool(ran[mode] != S))
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as fh:
                    fh.write(line + '\n')


if __name__ == '__main__':
    main()
