"""Timing of the autocovariance launch behind the convergence diagnostics (bh_autocov_sets, csrc/autocov.hip).

    python tools/convergence_bench.py [--repeats 5] [--out profiles/rNN_convergence.jsonl]

Leg (a) of the plan in DESIGN.md section 7f: bh_autocov_sets alone on run-length coded white-noise series made on the
device -- 16 x 2, 1 024 x 2 and 16 384 x 2 series (chains x halves) of n ~ 5e3 and 5e4 samples, 7 columns, 256 and
1 024 lags -- as fused multiply-adds per second (sum of n K ncols over the series / time) beside half of the 78.6 TFLOP/s
FP64 vector peak (one FMA is two flops).  Shapes whose matrix would not fit a tenth of the free device memory are left
out and said so.  The time is the whole call: the prefix sum of the weights, the launch, and the copy of the result to
the host.  Before timing, two calls must return equal bytes.  One JSON line per shape: the median of the repeats with
min and max.

Leg (b): StationPool.convergence() in one pass against its two comparators, on one finished pool of 4 stations x 16
chains whose sample arrays are tiled to 64 / 256 / 1 024 stations (the diagnostics read nothing but those arrays):
the loop over the station views (station(s).convergence() for every s), and the numpy restatement on the host -- the
expanded half chains, np.fft autocovariances and the rules, one station per task on 16 processes.  First the results
must agree: the loop's bit for bit, numpy's R-hat and tau to 1e-8.  Then >= 5 alternating repeats of each, medians with
min and max.  The loop over 1 024 views is timed on its first 64 stations and scaled, and says so in its line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayhunter_amd import _lib, convergence as cv  # noqa: E402

PEAK_FMA = 78.6e12 / 2
NCOLS = 7


def make(nseries, n, dev, seed=1):
    """nseries series of exactly n samples each: rows of weight 1 .. 4 (mean 2.5), the last row of a series clipped."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    rows = int(n / 2.5 * 1.05) + 8                                   # enough rows of mean weight 2.5 to pass n
    w = torch.randint(1, 5, (nseries, rows), generator=g, device=dev, dtype=torch.int64)
    cum = torch.cumsum(w, dim=1)
    assert int(cum[:, -1].min()) >= n
    w = torch.minimum(cum, torch.tensor(n, device=dev)) - torch.minimum(cum - w, torch.tensor(n, device=dev))
    D = torch.randn((nseries * rows, NCOLS), generator=g, device=dev, dtype=torch.float64)
    start = np.arange(nseries + 1, dtype=np.int64) * rows
    return D, w.reshape(-1).to(torch.int32).contiguous(), start


class Tiled(object):
    """The sample arrays of a finished StationPool repeated to `nstations` stations, behind what the diagnostics read
    of a StationPool: pool (the inner pool's attributes), chains_per_station, names, station(s)."""

    class Inner(object):
        pass

    def __init__(self, spool, nstations, first=0):
        src, c = spool.pool, spool.chains_per_station
        reps = -(-nstations // spool.nstations)
        inner = self.pool = Tiled.Inner()
        take = lambda a: np.concatenate([a] * reps)[first * c:(first + nstations) * c]
        for k in ('models', 'misfits', 'likes', 'noise', 'vpvs', 'iter'):
            setattr(inner, k, take(getattr(src, k)))
        counters = tuple(take(a) for a in src.counters())
        inner.counters = lambda: counters
        inner.nchains, inner.first = nstations * c, 0
        for k in ('iter_main', 'iter_burnin', 'ntargets', 'targets', 'initparams', 'priors'):
            setattr(inner, k, getattr(src, k))
        self.chains_per_station, self.nstations = c, nstations
        self.names = ['st%04d' % s for s in range(nstations)]

    def station(self, s):
        return Tiled(self, 1, first=s).pool

    def counters(self):
        return self.pool.counters()


def host_station(args):
    """The numpy restatement of one station: expanded half chains, np.fft autocovariances, the rules -> (rhat, tau) per
    column.  args: (columns [entries, K], w, series_start, n, nlags)."""
    D, w, start, n, nlags = args
    K = D.shape[1]
    S = len(start) - 1
    mean, acov = np.zeros((S, K)), np.zeros((S, K, nlags))
    for s in range(S):
        x = np.repeat(D[start[s]:start[s + 1]], w[start[s]:start[s + 1]], axis=0)
        mean[s] = x.mean(axis=0)
        f = np.fft.rfft(x - mean[s], n=2 * n, axis=0)
        acov[s] = (np.fft.irfft(f * np.conj(f), n=2 * n, axis=0)[:nlags] / n).T
    out = [cv.diagnose(mean[:, c], acov[:, c], n) for c in range(K)]
    return [d['rhat'] for d in out], [d['tau'] for d in out]


def host_restatement(tiled, nlags, procs, dev=1e9):
    from bayhunter_amd import selection as sel
    inner, c = tiled.pool, tiled.chains_per_station
    hs = sel.half_chain_series(inner, c, dev)            # the chains the one-pass form is given: none left out
    nt = inner.ntargets
    ci, ri = hs['ci'], hs['ri']
    cols = np.column_stack([inner.likes[ci, ri], inner.misfits[ci, ri], inner.vpvs[ci, ri], inner.noise[ci, ri],
                            (~np.isnan(inner.models[ci, ri])).sum(axis=1) / 2 - 1]).astype(np.float64)
    assert cols.shape[1] == 3 * nt + 4
    gs, ss = hs['group_start'], hs['series_start']
    tasks = []
    for g in range(gs.size - 1):
        lo, hi = ss[gs[g]], ss[gs[g + 1]]
        tasks.append((cols[lo:hi], hs['w'][lo:hi], ss[gs[g]:gs[g + 1] + 1] - lo, int(hs['n'][g]), nlags))
    return procs.map(host_station, tasks, chunksize=max(1, len(tasks) // 64))


def stations_leg(args, lines):
    import multiprocessing
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'scenarios'))
    from bayhunter_amd import convergence as conv
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from station_scenario import make_stations
    procs = multiprocessing.get_context('spawn').Pool(16)          # before the GPU is opened in this process's children
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=500, iter_main=args.main)
    stations = make_stations(os.path.join(root, 'tests', 'golden', 'tutorial_observed'), 4,
                             refs=case.get('refs', ('rdispph', 'prf')), yerr=True)
    with StationPool(stations, ip, case['priors'], chains_per_station=16, random_seeds=[1, 2, 3, 4],
                     nmodels=500 + args.main + 1) as spool:
        spool.run()
    kw = dict(nlags=args.nlags, dev=1e9, strict=False)
    for S in (64, 256, 1024):
        tiled = Tiled(spool, S)
        one = conv.stations_convergence(tiled, **kw)
        nloop = min(S, 64)
        loop = [conv.pool_convergence(tiled.station(s), nlags=args.nlags, dev=1e9) for s in range(nloop)]
        host = host_restatement(tiled, args.nlags, procs)
        cols = [c for c in one.columns if not one.stations[tiled.names[0]][c]['constant']]
        for s in range(nloop):
            for c in cols:
                a, b = one.stations[tiled.names[s]][c], loop[s][c]
                assert a['rhat'] == b['rhat'] and a['ess'] == b['ess'] and (a['tau'] == b['tau'] or np.isnan(a['tau']))
        for s in range(S):
            for i, c in enumerate(one.columns):
                if c in cols:
                    assert np.isclose(one.rhat[c][s], host[s][0][i], rtol=1e-8, atol=0, equal_nan=True), (s, c)
                    assert np.isclose(one.tau[c][s], host[s][1][i], rtol=1e-8, atol=0, equal_nan=True), (s, c)
        t = dict(one_pass=[], loop=[], host=[])
        for _ in range(max(5, args.repeats)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            conv.stations_convergence(tiled, **kw)
            t['one_pass'].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for s in range(nloop):
                conv.pool_convergence(tiled.station(s), nlags=args.nlags, dev=1e9)
            t['loop'].append((time.perf_counter() - t0) * S / nloop)
            t0 = time.perf_counter()
            host_restatement(tiled, args.nlags, procs)
            t['host'].append(time.perf_counter() - t0)
        line = dict(leg='stations', stations=S, chains=16, iter_main=args.main, nlags=args.nlags, n=int(one.stations[tiled.names[0]]['n']),
                    repeats=len(t['host']), loop_timed_on=nloop, host_processes=16, src=_lib.loaded_hash())
        for k, v in t.items():
            line.update({k + '_median': float(np.median(v)), k + '_min': min(v), k + '_max': max(v)})
        lines.append(line)
        print(json.dumps(line), flush=True)
    procs.close()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--legs', default='ab')
    ap.add_argument('--main', type=int, default=4000, help='main-phase iterations of leg (b)\'s pool')
    ap.add_argument('--nlags', type=int, default=1024)
    args = ap.parse_args()
    lines = []
    if 'b' in args.legs:
        stations_leg(args, lines)
    if 'a' in args.legs:
        kernel_leg(args, lines)
    if args.out:
        with open(args.out, 'w') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


def kernel_leg(args, lines):
    import torch
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for chains in (16, 1024, 16384):
        for n in (5000, 50000):
            S = 2 * chains
            need = S * (n / 2.5 * 1.05) * (8 * NCOLS + 8 * 4)
            free = torch.cuda.mem_get_info(dev)[0]
            if need > free / 10:
                lines.append(dict(leg='autocov', series=S, n=n, skipped='%.1f GB of rows' % (need / 1e9)))
                print(json.dumps(lines[-1]), flush=True)
                continue
            D, w, start = make(S, n, dev)
            mean = np.zeros((S, NCOLS))
            for K in (256, 1024):
                if S * NCOLS * K * 8 > 2 << 30:
                    lines.append(dict(leg='autocov', series=S, n=n, nlags=K, skipped='result above 2 GiB'))
                    print(json.dumps(lines[-1]), flush=True)
                    continue
                a, length = cv.autocov_sets(D, w, start, mean, K, stream)
                b, _ = cv.autocov_sets(D, w, start, mean, K, stream)
                assert np.all(length == n) and a.tobytes() == b.tobytes()
                ts = []
                for _ in range(max(5, args.repeats)):
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    cv.autocov_sets(D, w, start, mean, K, stream)
                    ts.append(time.perf_counter() - t0)
                fma = float(S) * NCOLS * sum(n - k for k in range(K))
                med = float(np.median(ts))
                lines.append(dict(leg='autocov', series=S, n=n, nlags=K, ncols=NCOLS, rows=int(D.shape[0]), seconds_median=med,
                                  seconds_min=min(ts), seconds_max=max(ts), repeats=len(ts), fma_per_s=fma / med,
                                  share_of_fp64_vector_peak=fma / med / PEAK_FMA, src=_lib.loaded_hash()))
                print(json.dumps(lines[-1]), flush=True)
            del D, w
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
