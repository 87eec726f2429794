"""What the Moho statistics cost (bayhunter_amd/moho.py), one process, every leg warmed once and the median of
--repeats (default 5) reported; one JSON line per leg.

  (a) moho.summarize on --rows (default 10^6) weighted rows against the reference's way on the host: the per-model
      loop of plot_moho_crustvel_tradeoff as tests/moho_ref.py restates it, on the rows repeated by their weights.
      The loop is timed on --host-rows (default 10^4) unweighted rows and scaled to the weighted total, and the
      line says so (host_scaled_from).
  (b) StationPool.moho() at 64, 256 and 1 024 stations x 16 chains against the loop over pool.station(s).moho() on the
      same finished pool, after asserting that the two agree (counts and order statistics exactly, mean and std to
      tests/posterior_tolerances.py).

    python tools/moho_bench.py [--legs a,b] [--configs 64x16 256x16 1024x16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='a,b')
    ap.add_argument('--rows', type=int, default=1000000)
    ap.add_argument('--host-rows', type=int, default=10000)
    ap.add_argument('--configs', nargs='*', default=['64x16', '256x16', '1024x16'])
    ap.add_argument('--iters', type=int, default=120)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--mohovs', type=float, default=3.8)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, 'tests', 'scenarios'), os.path.join(here, 'tests'), here):
        sys.path.insert(0, p)
    import torch
    import moho_ref as ref
    from posterior_tolerances import MEAN_RTOL, STD_ATOL, STD_RTOL
    from bayhunter_amd import _lib, moho

    def emit(d):
        d = dict(d, tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats)
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def median_of(fn):
        timed(fn)                                            # warm
        secs = [timed(fn)[0] for _ in range(args.repeats)]
        return float(np.median(secs)), secs

    if 'a' in args.legs.split(','):
        rs = np.random.RandomState(1)
        window, mohovs = (20., 50.), 4.1
        base = ref.random_rows(rs, 20000, 40, np.float32)
        rows = base[rs.randint(0, base.shape[0], args.rows)]
        w = rs.randint(0, 300, args.rows).astype(np.int32)
        trows, tw = torch.from_numpy(rows).cuda(), torch.from_numpy(w).cuda()
        dev_s, dev_all = median_of(lambda: moho.summarize(trows, tw, window, mohovs))
        up_s, _ = median_of(lambda: moho.summarize(rows, w, window, mohovs))        # host arrays: the upload included
        res = moho.summarize(trows, tw, window, mohovs)
        hrows = rows[:args.host_rows]
        t0 = time.perf_counter()
        D = ref.derive(hrows, window, mohovs)
        loop_s = time.perf_counter() - t0
        assert np.array_equal(D, moho.derive(trows[:args.host_rows], window[0], window[1], mohovs,
                                             torch.cuda.current_stream().cuda_stream).cpu().numpy(), equal_nan=True)
        total = int(w.astype(np.int64).sum())
        emit(dict(bench='moho_summarize', rows=args.rows, weight_total=total, nmodels=res['nmodels'],
                  nexcluded=res['nexcluded'], device_median_s=round(dev_s, 5), device_s=[round(x, 5) for x in dev_all],
                  device_with_upload_median_s=round(up_s, 5), host_loop_rows=args.host_rows,
                  host_loop_s=round(loop_s, 4), host_us_per_row=round(1e6 * loop_s / args.host_rows, 2),
                  host_scaled_from='the per-model loop of tests/moho_ref.py timed on host_loop_rows rows, scaled',
                  host_s_per_stored_row_scaled=round(loop_s / args.host_rows * args.rows, 2),
                  host_s_per_expanded_row_scaled=round(loop_s / args.host_rows * total, 1),
                  speedup_vs_stored_rows=round(loop_s / args.host_rows * args.rows / dev_s, 1),
                  speedup_vs_expanded_rows=round(loop_s / args.host_rows * total / dev_s, 1)))

    if 'b' in args.legs.split(','):
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
                        out[name] = pool.station(name).moho(mohovs=args.mohovs)
                    except ValueError:
                        out[name] = None
                return out

            one = lambda: pool.moho(mohovs=args.mohovs)
            want, got = loop(), one()
            for s, name in enumerate(pool.names):
                r = want[name]
                if r is None:
                    assert got.nmodels[s] == 0 or name in got.failed, name
                    continue
                assert got.nmodels[s] == r['nmodels'] and got.nexcluded[s] == r['nexcluded'], name
                for q in moho.NAMES:
                    assert all(getattr(got, q)[k][s] == r[q][k] for k in ('median', 'min', 'max')), (name, q)
                    np.testing.assert_allclose(getattr(got, q)['mean'][s], r[q]['mean'], rtol=MEAN_RTOL, atol=0)
                    np.testing.assert_allclose(getattr(got, q)['std'][s], r[q]['std'], rtol=STD_RTOL, atol=STD_ATOL)
            loop_s, loop_all = median_of(loop)
            one_s, one_all = median_of(one)
            emit(dict(bench='station_moho', stations=S, chains_per_station=c, iterations=iters + iters // 2,
                      models=int(got.nmodels.sum() + got.nexcluded.sum()), stations_with_moho=int((got.nmodels > 0).sum()),
                      equal=True, loop_s=[round(x, 4) for x in loop_all], one_call_s=[round(x, 4) for x in one_all],
                      loop_median_s=round(loop_s, 4), one_call_median_s=round(one_s, 4),
                      loop_ms_per_station=round(1e3 * loop_s / S, 3), speedup=round(loop_s / one_s, 2)))


if __name__ == '__main__':
    main()
