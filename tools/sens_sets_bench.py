"""What the posterior sensitivity kernels cost (bayhunter_amd/sensitivity.py, csrc/sens_sets.hip), one process, every leg
warmed once, the median of --repeats (default 7) device-synchronised wall times reported with every run; one JSON line
per leg, appended to profiles/sens_sets.jsonl and stamped with the hash of the loaded library.

  (a) the reduction alone (bh_sens_sets_create + add + finish with its copies to the host) against the bh_sens_batch call
      that precedes it, on the same --rows (default 65 536) ten-layer models of bayhunter_amd.synthetic.draw_models, 21
      periods, 200 depth bins, kind 'vs_total', integer weights, as 1 set and as 256 sets.
  (b) StationPool.sensitivity() at --configs (default 16x8: stations x chains) against the loop over
      pool.station(s).sensitivity() on the same finished pool, after asserting that the two agree bit for bit.
  (c) StationPool.sensitivity() against the numpy restatement (sensitivity.batch + vs_total + to_depth per row) on one
      host core: the device pass of `batch` is not counted, the host part (vs_total, to_depth, the weighted moments) is
      timed on the first --host-rows (default 2 000) rows and scaled to all of them, and the line says so.

    python tools/sens_sets_bench.py [--legs a,b,c] [--rows 65536] [--configs 16x8] [--out FILE]
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
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--nper', type=int, default=21)
    ap.add_argument('--bins', type=int, default=200)
    ap.add_argument('--configs', nargs='*', default=['16x8'])
    ap.add_argument('--iters', type=int, default=120)
    ap.add_argument('--host-rows', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=os.path.join(here, 'profiles', 'sens_sets.jsonl'))
    args = ap.parse_args()
    for p in (os.path.join(here, 'tests', 'scenarios'), os.path.join(here, 'tests'), here):
        sys.path.insert(0, p)
    import torch
    from bayhunter_amd import _lib, sensitivity as sens
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
        from bayhunter_amd.engine import ForwardEngine, SwdSpec
        from bayhunter_amd.synthetic import draw_models
        B = args.rows
        per = np.linspace(1, 41, args.nper)
        edges = np.linspace(0., 100., args.bins + 1)
        H, VP, VS, RHO, nl = draw_models(B, args.layers, seed=1)
        eng = ForwardEngine(swd=[SwdSpec('rdispph', per)])
        models = eng.upload(H, VP, VS, RHO, nl)
        out, err = eng.alloc_out(B)
        search = runs_of(lambda: eng.run(models, out=out, err=err))
        pass_ = runs_of(lambda: eng.sensitivity(models, out=out, err=err))
        res = eng.sensitivity(models, out=out, err=err)
        q = (models.VP / models.VS).contiguous()
        w = torch.from_numpy(np.random.RandomState(2).randint(0, 300, B).astype(np.int32)).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        for nsets in (1, 256):
            start = np.linspace(0, B, nsets + 1).astype(np.int64)

            def reduce():
                with sens.SensSets(start, per.size, edges, _lib.SENS_KINDS['vs_total'], 0.32, stream) as hd:
                    hd.add(0, models, res['K'], res['c'], q, w)
                    return hd.finish()
            r = runs_of(reduce)
            sums = reduce()
            emit(dict(bench='sens_sets_reduction', rows=B, layers=args.layers, nper=args.nper, bins=args.bins, sets=nsets,
                      kind='vs_total', reduction=r, sens_batch=pass_, search=search,
                      reduction_over_sens_batch=round(r['median_s'] / pass_['median_s'], 4),
                      rows_per_s=round(B / r['median_s']), weight_total=int(sums['total'][:, 0].sum()),
                      weight_excluded=int(sums['excluded'][:, 0].sum()),
                      not_measured=['other layer counts, period counts and bin counts', 'sets cut over several add calls']))

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
                        out[name] = pool.station(name).sensitivity()
                    except ValueError:
                        out[name] = None
                return out

            one = lambda: pool.sensitivity()
            want, got = loop(), one()
            for name in pool.names:
                if want[name] is None:
                    assert name not in got.stations, name
                    continue
                for k, v in want[name].items():
                    assert np.asarray(v).tobytes() == np.asarray(got.stations[name][k]).tobytes(), (name, k)
            ci, ri, w, set_start, _ = sel.station_rows(pool.pool, c)
            common = dict(stations=S, chains_per_station=c, iterations=iters + iters // 2, rows=int(set_start[-1]),
                          stations_with_models=len(got.stations), nper=int(got.periods.size), bins=int(got.edges.size - 1))
            one_r = runs_of(one)
            if 'b' in legs:
                loop_r = runs_of(loop)
                emit(dict(bench='station_sensitivity_vs_views', equal=True, one_call=one_r, loop=loop_r,
                          loop_ms_per_station=round(1e3 * loop_r['median_s'] / S, 3),
                          speedup=round(loop_r['median_s'] / one_r['median_s'], 2), **common))
            if 'c' in legs:
                from bayhunter_amd import datafits as df
                from bayhunter_amd.models import layers_from_voronoi
                n = min(args.host_rows, int(set_start[-1]))
                rows = torch.from_numpy(pool.pool.models[ci[:n], ri[:n]].astype(np.float64)).cuda()
                vsn, zv, nlay = df._layers(rows, rows.device)
                dm, _ = layers_from_voronoi(vsn, zv, nlay, torch.from_numpy(pool.pool.vpvs[ci[:n], ri[:n]].astype(np.float64)).cuda(),
                                            df._OPEN_PRIORS, mantle=pool.pool.priors.get('mantle'))
                Hh, VPh, VSh, RHOh = (dm.packed[:, k, :].cpu().numpy() for k in range(4))
                nl = dm.nlay.cpu().numpy()
                res = sens.batch(got.periods, Hh, VPh, VSh, RHOh, nl, 'rayleigh')
                wn = w[:n].astype(np.float64)

                def host():
                    with np.errstate(invalid='ignore', divide='ignore'):
                        G = sens.vs_total(res['K'], (VPh / VSh)[:, None, :])
                    x = np.zeros((n, got.periods.size, got.edges.size))
                    for r in range(n):
                        m = int(nl[r])
                        if m >= 2:
                            x[r, :, :-1], x[r, :, -1] = sens.to_depth(G[r][:, :m], Hh[r, :m], got.edges)
                    ok = ~np.isnan(res['c'])
                    W = (wn[:, None] * ok).sum(axis=0)
                    xz = np.where(ok[:, :, None], x, 0.)
                    mean = np.einsum('r,rpc->pc', wn, xz) / W[:, None]
                    var = np.einsum('r,rpc->pc', wn, xz * xz) / W[:, None] - mean * mean
                    return mean, var, xz.min(axis=0), xz.max(axis=0)
                secs = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    host()
                    secs.append(time.perf_counter() - t0)
                host_s = float(np.median(secs))
                frac = float(n) / max(1, int(set_start[-1]))
                emit(dict(bench='station_sensitivity_vs_numpy', one_call=one_r, host_rows=n, host_median_s=round(host_s, 4),
                          host_min_s=round(min(secs), 4), host_max_s=round(max(secs), 4),
                          host_scaled_from='vs_total + to_depth + weighted moments in numpy on one core, timed on host_rows '
                                           'rows, scaled by rows; the device pass that makes K is not counted',
                          host_scaled_s=round(host_s / frac, 3), speedup=round(host_s / frac / one_r['median_s'], 1),
                          **common))


if __name__ == '__main__':
    main()
