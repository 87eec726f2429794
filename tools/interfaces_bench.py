"""What the discontinuity statistics cost (bayhunter_amd/interfaces.py), one process, every leg warmed once, the median
of --repeats (default 7) runs reported with their spread (min, max and every run); one JSON line per leg, appended to
profiles/interfaces.jsonl.

  (a) bh_interfaces_sets alone on --rows (default 10^6) device-resident float32 rows of width 42 with integer
      weights, as 1 set and as 256 sets, over the default table (100 depth x 40 jump bins, one group of depth bins)
      and over 400 x 64 bins (four groups).  Timed is the whole call: the count launch, the two moment launches with
      their slab reductions, and the copies of the result to the host.
  (b) StationPool.interfaces() at --configs (default 64x16: stations x chains) against the loop over
      pool.station(s).interfaces() on the same finished pool, after asserting that the two agree field for field.
  (c) StationPool.interfaces() against the numpy restatement (tests/interfaces_ref.py) on one host core, station
      after station on the same rows.  The restatement is timed on the first --host-stations (default 8) stations and
      scaled to all of them, and the line says so.

    python tools/interfaces_bench.py [--legs a,b,c] [--configs 64x16 256x16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='a,b,c')
    ap.add_argument('--rows', type=int, default=1000000)
    ap.add_argument('--configs', nargs='*', default=['64x16'])
    ap.add_argument('--iters', type=int, default=120)
    ap.add_argument('--host-stations', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=os.path.join(here, 'profiles', 'interfaces.jsonl'))
    args = ap.parse_args()
    for p in (os.path.join(here, 'tests', 'scenarios'), os.path.join(here, 'tests'), here):
        sys.path.insert(0, p)
    import torch
    import interfaces_ref as ref
    from bayhunter_amd import _lib, interfaces
    from bayhunter_amd import selection as sel
    legs = args.legs.split(',')

    def emit(d):
        d = dict(d, tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats, device=torch.cuda.get_device_name(0))
        line = json.dumps(d)
        print(line, flush=True)
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def runs_of(fn):
        timed(fn)                                            # warm
        secs = [timed(fn)[0] for _ in range(args.repeats)]
        return dict(median_s=round(float(np.median(secs)), 6), min_s=round(min(secs), 6), max_s=round(max(secs), 6),
                    runs_s=[round(x, 6) for x in secs])

    if 'a' in legs:
        rs = np.random.RandomState(1)
        base = ref.random_rows(rs, 20000, 42, np.float32)
        rows = base[rs.randint(0, base.shape[0], args.rows)]
        w = rs.randint(0, 300, args.rows).astype(np.int32)
        trows, tw = torch.from_numpy(rows).cuda(), torch.from_numpy(w).cuda()
        dev = trows.device
        tables = {'100x40': interfaces._edges(None, None),
                  '400x64': (np.arange(401) * 0.25, -2. + np.arange(65) * 0.0625)}
        for nsets in (1, 256):
            start = np.linspace(0, args.rows, nsets + 1).astype(np.int64)
            for name, (de, je) in tables.items():
                r = runs_of(lambda: interfaces._reduce(dev, trows, tw, start, de, je))
                res = interfaces._reduce(dev, trows, tw, start, de, je)
                emit(dict(bench='interfaces_sets_call', rows=args.rows, width=42, dtype='float32', sets=nsets, table=name,
                          depth_bin_groups=-(-(de.size - 1) // (60 * 1024 // (8 * (6 + je.size - 1)))),
                          interfaces=int(res['count'].sum()), weight_total=int(res['total'].sum()),
                          rows_per_s=round(args.rows / r['median_s']), **r))

    if 'b' in legs or 'c' in legs:
        from chain_scenario import CASES
        from station_scenario import make_stations
        from bayhunter_amd.stations import StationPool
        case = CASES['tutorial']
        data = os.path.join(here, 'tests', 'golden', 'tutorial_observed')
        for cfg in args.configs:
            S, c = (int(v) for v in cfg.lower().split('x'))
            iters = args.iters
            seeds = np.asarray([[np.random.RandomState(s).randint(1000) for _ in range(c)] for s in range(S)])
            ip = dict(case['initparams'], iter_burnin=iters, iter_main=iters // 2, acceptance=(40, 100))
            with StationPool(make_stations(data, S, yerr=True), ip, case['priors'], seeds=seeds,
                             nmodels=iters + iters // 2 + 1) as pool:
                pool.run()

            def loop():
                out = {}
                for name in pool.names:
                    try:
                        out[name] = pool.station(name).interfaces()
                    except ValueError:
                        out[name] = None
                return out

            one = lambda: pool.interfaces()
            want, got = loop(), one()
            for name in pool.names:
                if want[name] is None:
                    assert name not in got.stations, name
                    continue
                for k, v in want[name].items():
                    assert np.array_equal(v, got.stations[name][k], equal_nan=True), (name, k)
            common = dict(stations=S, chains_per_station=c, iterations=iters + iters // 2,
                          stations_with_models=len(got.stations), interfaces=int(np.nansum(got.count)))
            one_r = runs_of(one)
            if 'b' in legs:
                loop_r = runs_of(loop)
                emit(dict(bench='station_interfaces_vs_views', equal=True, one_call=one_r, loop=loop_r,
                          loop_ms_per_station=round(1e3 * loop_r['median_s'] / S, 3),
                          speedup=round(loop_r['median_s'] / one_r['median_s'], 2), **common))
            if 'c' in legs:
                ci, ri, w, set_start, _ = sel.station_rows(pool.pool, c)
                rows = pool.pool.models[ci, ri]
                de, je = interfaces._edges(None, None)
                H = min(args.host_stations, S)

                def host():
                    return [ref.summarize(rows[set_start[z]:set_start[z + 1]], w[set_start[z]:set_start[z + 1]], de, je)
                            for z in range(H)]
                for z, r in enumerate(host()):
                    name = pool.names[z]
                    if name in got.stations:
                        assert np.array_equal(r['count'], got.stations[name]['count']), name
                        assert np.array_equal(r['models_neg'], got.stations[name]['models_neg']), name
                secs = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    host()
                    secs.append(time.perf_counter() - t0)
                host_s = float(np.median(secs))
                frac = float(set_start[H]) / max(1, int(set_start[-1]))
                emit(dict(bench='station_interfaces_vs_numpy', one_call=one_r, host_stations=H, host_rows=int(set_start[H]),
                          rows=int(set_start[-1]), weight_total=int(w.sum()), host_median_s=round(host_s, 4),
                          host_min_s=round(min(secs), 4), host_max_s=round(max(secs), 4),
                          host_scaled_from='tests/interfaces_ref.py on one core, timed on host_rows rows, scaled by rows',
                          host_scaled_s=round(host_s / frac, 3), speedup=round(host_s / frac / one_r['median_s'], 1),
                          **common))


if __name__ == '__main__':
    main()
