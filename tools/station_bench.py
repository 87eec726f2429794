"""GPU box: what putting many stations into one chain pool buys, on the tutorial inversion (Rayleigh phase + P-RF, free
vp/vs and noise, like tools/chain_bench.py).  For S stations of c chains each, three ways to run the S * c chains:

    stations   one StationPool of S x c chains, every station its own observed data
    onepool    one ChainPool of S * c chains on ONE station (the pool's speed when no observation sets are involved;
               with --root pointing at a checkout of another commit: that commit's pool, for before/after)
    singles    S single-station ChainPools of c chains, one after the other -- what is done without the feature.
               For S > --sample only --sample of them are timed and the time is scaled by S / --sample (said in
               the output: "scaled": true)

    python tools/station_bench.py [--modes stations,onepool,singles] [--repeats 5] [--sample 16] [--root DIR]
                                  [--vary-p LO HI] [--gaps FRACTION] [--posterior | --datafits | --scalars] [--out FILE.jsonl]
                                  [SxC ...]
                                  (default 64x16 256x16 1024x16 1024x4)

--vary-p LO HI: every station its own receiver-function ray parameter, spread evenly over [LO, HI] s/deg; the station
pool runs with per_station=('p',) (the per-row form of rf_kernel), the single pools each at their station's p, `onepool`
at station 0's.

--gaps FRACTION: every station but station 0 lacks that fraction of its dispersion periods (its own random draw, at
least one period kept; NaN in obsdata.y) and the station pool runs with missing='mask' (like_gaps_kernel); `singles` are
one-station StationPools with missing='mask', `onepool` runs on station 0, which is complete.  --gaps 0 takes the
same code path with no gap anywhere: the full-mask cost, to set against a tree without the feature (--root), which
is run without the keyword.  Every line carries the library's source hash.

--posterior: instead of the three ways to run, what reading the result costs.  One finished StationPool of S x c chains
is summarised twice: by the loop over its station views (pool.station(s).posterior(), one pair of handles per station)
and by StationPool.posterior() (one pass over all stations).  Each is warmed once, then timed --repeats times
wall-clock around a device synchronisation; the two results are asserted equal, field by field and bit for bit,
before a time is reported.  One JSON line per S x c.

--datafits: the same for the statistics of the modelled data: the loop over pool.station(s).datafits() (one forward
pass and one bh_datafits handle per station) against StationPool.datafits() (one forward pass and one bh_datafits_sets
handle for all stations); with --vary-p the pool has per_station=('p',).

--scalars: the same for the posterior of the sampler's scalar parameters: the loop over pool.station(s).scalars() (one
bh_datafits handle and one bh_hist2d_sets call per station) against StationPool.scalars() (one bh_datafits_sets handle
and one bh_hist2d_sets launch for all stations), both with the Moho column and the pairs (moho, vpvs), (sigma of the
second target, sigma of the first) and (nlayers, like).

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
    ap.add_argument('configs', nargs='*', default=None,
                    help='default 64x16 256x16 1024x16 1024x4 (with --posterior: 64x16 256x16 1024x16)')
    ap.add_argument('--modes', default='stations,onepool,singles')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sample', type=int, default=16)
    ap.add_argument('--iters', type=int, default=None, help='burn-in iterations (main phase: half of it)')
    ap.add_argument('--root', default=None, help='tree whose bayhunter_amd is measured (default: this one)')
    ap.add_argument('--vary-p', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                    help="stations with p spread evenly over [LO, HI] s/deg, pooled with per_station=('p',)")
    ap.add_argument('--gaps', type=float, default=None, metavar='FRACTION',
                    help="fraction of the dispersion periods missing at every station but the first; pooled with missing='mask'")
    ap.add_argument('--posterior', action='store_true',
                    help='time StationPool.posterior() against the loop over station views on one finished pool')
    ap.add_argument('--datafits', action='store_true',
                    help='time StationPool.datafits() against the loop over station views on one finished pool')
    ap.add_argument('--scalars', action='store_true',
                    help='time StationPool.scalars() against the loop over station views on one finished pool')
    ap.add_argument('--tag', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not args.configs:
        args.configs = ['64x16', '256x16', '1024x16'] + ([] if args.posterior or args.datafits or args.scalars else ['1024x4'])
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
    import inspect
    from bayhunter_amd.stations import StationPool
    mask = dict(missing='mask') if args.gaps is not None and 'missing' in inspect.signature(StationPool.__init__).parameters else {}
    assert mask or not args.gaps, 'this tree has no StationPool(missing=...)'
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
            with StationPool(stations, ip, case['priors'], seeds=seeds, **per, **mask, **kw) as pool:
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
            single = StationPool(stations[s:s + 1], ip, case['priors'], seeds=seeds[s:s + 1], **mask, **kw) if args.gaps \
                else ChainPool(stations[s], ip, case['priors'], seeds=seeds[s], **kw)
            with single as pool:
                t0 = time.perf_counter()
                pool.run()
                dt += time.perf_counter() - t0
        return dt, k

    def same(a, b, path=''):
        """every leaf of two result trees equal (NaN = NaN)"""
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + '/' + str(k))
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, '%s[%d]' % (path, i))
        else:
            x, y = np.asarray(a), np.asarray(b)
            assert np.array_equal(x, y, equal_nan=x.dtype.kind in 'fc'), path

    def readout_leg(what, S, c, iters, stations):
        """what: 'posterior', 'datafits' or 'scalars' -- the method of the station views and of the pool"""
        import torch
        from bayhunter_amd.stations import StationPool
        per = dict(per_station=('p',)) if args.vary_p else {}
        with StationPool(stations, params(iters), case['priors'], seeds=seeds_of(S, c), nmodels=iters + iters // 2 + 1,
                         **per) as pool:
            pool.run()

        kw = {}
        if what == 'scalars':
            refs = [t.ref for t in stations[0].targets]
            kw = dict(moho=case['priors']['z'], pairs=[('moho', 'vpvs'), ('sigma:%s' % refs[1], 'sigma:%s' % refs[0]),
                                                       ('nlayers', 'like')])

        def loop():
            out, failed = {}, {}
            for name in pool.names:
                try:
                    out[name] = getattr(pool.station(name), what)(**kw)
                except (ValueError, bayhunter_amd._lib.BayHunterAmdError) as e:
                    failed[name] = str(e)
            return out, failed

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r

        one = lambda: getattr(pool, what)(strict=False, **kw)
        (_, (want, wfailed)), (_, got) = timed(loop), timed(one)       # warm
        assert sorted(got.failed) == sorted(wfailed) and list(got.stations) == list(want), (got.failed, wfailed)
        same(got.stations, want)
        secs = dict(loop=[], one_call=[])
        for _ in range(args.repeats):
            secs['loop'].append(timed(loop)[0])
            secs['one_call'].append(timed(one)[0])
        med = {k: float(np.median(v)) for k, v in secs.items()}
        return dict(bench='station_' + what, tag=args.tag, src=bayhunter_amd._lib.built_hash(), vary_p=args.vary_p, stations=S, chains_per_station=c, chains=S * c,
                    iterations=iters + iters // 2, models=int(sum(r['nmodels'] for r in want.values())),
                    stations_failed=len(wfailed), equal=True, repeats=args.repeats,
                    loop_s=[round(x, 4) for x in secs['loop']], one_call_s=[round(x, 4) for x in secs['one_call']],
                    loop_median_s=round(med['loop'], 4), one_call_median_s=round(med['one_call'], 4),
                    loop_ms_per_station=round(1e3 * med['loop'] / S, 3), speedup=round(med['loop'] / med['one_call'], 2))

    for cfg in args.configs:
        S, c = (int(v) for v in cfg.lower().split('x'))
        iters = args.iters or (120 if S * c <= 4096 else 60)
        stations = make_stations(data, S, yerr=True)
        if args.vary_p:
            for joint, p in zip(stations, np.linspace(args.vary_p[0], args.vary_p[1], S)):
                joint.targets[1].moddata.plugin.set_modelparams(p=float(p))
        if args.posterior or args.datafits or args.scalars:
            line = json.dumps(readout_leg('posterior' if args.posterior else 'datafits' if args.datafits else 'scalars',
                                          S, c, iters, stations))
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as fh:
                    fh.write(line + '\n')
            continue
        if args.gaps:
            for s, joint in enumerate(stations[1:], 1):
                y = joint.targets[0].obsdata.y.copy()
                miss = np.random.RandomState(5000 + s).uniform(size=y.size) < args.gaps
                miss[np.random.RandomState(7000 + s).randint(y.size)] = False
                y[miss] = np.nan
                joint.targets[0].obsdata.y = y
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
            rec = dict(bench='station_pool', tag=args.tag, src=bayhunter_amd._lib.built_hash(), vary_p=args.vary_p, gaps=args.gaps,
                       mode=mode, stations=S, chains_per_station=c, chains=S * c,
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
