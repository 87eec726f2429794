"""Timing of the depth-to-depth covariance (bh_depthcov_sets, csrc/depthcov.hip; bayhunter_amd/covariance.py).

    python tools/depthcov_bench.py [--repeats 5] [--legs ab] [--out profiles/rNN_depthcov.jsonl]   (--out appends)

Leg (a): bh_depthcov_sets alone on random models made on the device -- 1e5, 1e6 and 4e6 rows of 2 .. 12 nuclei in 1, 64
and 1 024 sets, 201 depths and one extra column (K = 202: 13 x 13 tiles, 91 tile pairs), float32 rows with weights
1 .. 40.  The time is the whole call: the uploads of the grid and the centres, the launches, the fold, and the copy of S
[sets, K, K] to the host.  Reported: the median of the repeats with min and max, the flops of the MFMAs issued (one
v_mfma_f64_16x16x4_f64 of 2 048 flops per tile pair and four rows) per second, and that as a share of 78.6 TFLOP/s,
the FP64 matrix peak AMD publishes for the MI355X.  Before timing, two calls must return equal bytes.

Leg (b): StationPool.depth_covariance() in one pass against np.cov(X.T, fweights=w, bias=True) per station on the host,
on one finished pool of 4 stations x 8 chains whose sample arrays are tiled to 64 and 256 stations.  The host side is
timed twice: np.cov alone on matrices X made beforehand, and with the making of X (numpy's interpolation of every row
onto the grid).  First the covariances must agree to 1e-9 of the variances' scale.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bayhunter_amd import _lib, covariance as cov, convergence as conv, selection as sel  # noqa: E402

PEAK_FP64_MATRIX = 78.6e12
WIDTH, NDEP = 40, 201


def make_rows(R, dev, seed=1):
    """R float32 rows [vs(n) | z(n) | NaN ..] of WIDTH columns, n = 2 .. 12 nuclei, weights 1 .. 40, one extra column."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    half = WIDTH // 2
    vs = torch.rand((R, half), generator=g, device=dev) * 3 + 2
    z = torch.sort(torch.rand((R, half), generator=g, device=dev) * 60, dim=1)[0]
    n = torch.randint(2, 13, (R, 1), generator=g, device=dev)
    j = torch.arange(WIDTH, device=dev)[None, :]
    src = torch.cat((vs, z), dim=1)
    idx = torch.where(j < n, j, torch.clamp(j - n, 0, half - 1) + half)
    rows = torch.where(j < 2 * n, torch.gather(src, 1, idx), torch.tensor(float('nan'), device=dev))
    w = torch.randint(1, 41, (R,), generator=g, device=dev, dtype=torch.int32)
    extra = torch.rand((R, 1), generator=g, device=dev, dtype=torch.float64) * 0.3 + 1.6
    return rows.contiguous(), w, extra


def kernel_leg(args, lines):
    import torch
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    dep = np.linspace(0, 100, NDEP)
    K = NDEP + 1
    npairs = (-(-K // 16)) * (-(-K // 16) + 1) // 2
    for R in (100000, 1000000, 4000000):
        rows, w, extra = make_rows(R, dev)
        for Z in (1, 64, 1024):
            start = (np.arange(Z + 1, dtype=np.int64) * R) // Z
            center = np.tile(np.r_[np.full(NDEP, 3.5), 1.75], (Z, 1))
            a = cov.depthcov_sets(rows, w, extra, start, dep, center, stream)
            b = cov.depthcov_sets(rows, w, extra, start, dep, center, stream)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and int(a[2].sum()) == int(w.sum())
            ts = []
            for _ in range(max(5, args.repeats)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                cov.depthcov_sets(rows, w, extra, start, dep, center, stream)
                ts.append(time.perf_counter() - t0)
            blocks = int(np.sum(-(-np.diff(start) // _lib.DEPTHCOV_BLOCK_ROWS)))
            flops = 2048. * npairs * sum(-(-min(_lib.DEPTHCOV_BLOCK_ROWS, int(n) - b0) // 4) for n in np.diff(start)
                                         for b0 in range(0, int(n), _lib.DEPTHCOV_BLOCK_ROWS))
            med = float(np.median(ts))
            lines.append(dict(leg='depthcov', rows=R, sets=Z, K=K, tile_pairs=npairs, blocks=blocks, seconds_median=med,
                              seconds_min=min(ts), seconds_max=max(ts), repeats=len(ts), mfma_flops=flops,
                              tflops=flops / med / 1e12, share_of_fp64_matrix_peak=flops / med / PEAK_FP64_MATRIX,
                              result_bytes=Z * K * K * 8, src=_lib.loaded_hash()))
            print(json.dumps(lines[-1]), flush=True)
        del rows, w, extra
        torch.cuda.empty_cache()


def host_matrices(tiled, dep, extras_of):
    """Per station (X [rows, K], w) of the rows the one-pass form takes (no chain left out)."""
    inner, c = tiled.pool, tiled.chains_per_station
    ci, ri, w, set_start, _ = sel.station_rows(inner, c, 'weighted', 1e9, True)
    out = []
    for z in range(set_start.size - 1):
        a, b = int(set_start[z]), int(set_start[z + 1])
        X = np.column_stack((conv.vs_at(inner.models[ci[a:b], ri[a:b]], dep), extras_of(inner, ci[a:b], ri[a:b])))
        out.append((X, w[a:b]))
    return out


def stations_leg(args, lines):
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'scenarios'))
    from bayhunter_amd.stations import StationPool
    from chain_scenario import CASES
    from convergence_bench import Tiled
    from station_scenario import make_stations
    case = CASES['tutorial']
    ip = dict(case['initparams'], iter_burnin=300, iter_main=args.main)
    stations = make_stations(os.path.join(ROOT, 'tests', 'golden', 'tutorial_observed'), 4,
                             refs=case.get('refs', ('rdispph', 'prf')), yerr=True)
    with StationPool(stations, ip, case['priors'], chains_per_station=8, random_seeds=[1, 2, 3, 4],
                     nmodels=300 + args.main + 1) as spool:
        spool.run()
    dep = np.linspace(0, 100, NDEP)
    vpvs = lambda inner, ci, ri: inner.vpvs[ci, ri].astype(np.float64)
    kw = dict(extras=('vpvs',), dev=1e9, strict=False)
    for S in (64, 256):
        tiled = Tiled(spool, S)
        one = cov.stations_depth_covariance(tiled, **kw)
        mats = host_matrices(tiled, dep, vpvs)
        for s in range(S):
            want = np.cov(mats[s][0].T, fweights=mats[s][1], bias=True)
            scale = np.sqrt(np.outer(np.diag(want), np.diag(want))).max()
            assert np.abs(one.cov[s] - want).max() <= 1e-9 * scale, s
        t = dict(one_pass=[], host_cov=[], host_all=[])
        for _ in range(max(5, args.repeats)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cov.stations_depth_covariance(tiled, **kw)
            t['one_pass'].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for X, w in mats:
                np.cov(X.T, fweights=w, bias=True)
            t['host_cov'].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for X, w in host_matrices(tiled, dep, vpvs):
                np.cov(X.T, fweights=w, bias=True)
            t['host_all'].append(time.perf_counter() - t0)
        line = dict(leg='stations', stations=S, chains=8, iter_main=args.main, K=NDEP + 1,
                    rows=int(sum(m[0].shape[0] for m in mats)), models=int(one.nmodels.sum()), repeats=len(t['one_pass']),
                    host_processes=1, src=_lib.loaded_hash())
        for k, v in t.items():
            line.update({k + '_median': float(np.median(v)), k + '_min': min(v), k + '_max': max(v)})
        lines.append(line)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--legs', default='ab')
    ap.add_argument('--main', type=int, default=1500, help='main-phase iterations of leg (b)\'s pool')
    args = ap.parse_args()
    lines = []
    if 'a' in args.legs:
        kernel_leg(args, lines)
    if 'b' in args.legs:
        stations_leg(args, lines)
    if args.out:
        with open(args.out, 'a') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
