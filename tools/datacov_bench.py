"""Timing of the cross-covariance of Vs(z) and the modelled data (bh_datacov_sets, csrc/datacov.hip;
bayhunter_amd/datacov.py).

    python tools/datacov_bench.py [--repeats 5] [--legs ab] [--out profiles/datacov.jsonl]   (--out appends)

Leg (a): bh_datacov_sets alone on random models and synthetic data made on the device -- 1e6 rows of 2 .. 12 nuclei in 1
and 256 sets, 201 depths and one extra column (K = 202: 13 tiles) against S = 222 data columns (21 periods and a
201-sample receiver function: 14 tiles, two groups of 7), float32 rows with weights 1 .. 40, one flag column with about
1 % of the rows flagged.  The time is the whole call: the uploads of the grid and the centres, the pre-pass, the
launches, the fold, and the copy of C [sets, K, S] to the host.  Reported: the median of the repeats with min and max,
the flops of the MFMAs issued (one v_mfma_f64_16x16x4_f64 of 2 048 flops per tile pair and four rows) per second, and
that as a share of 78.6 TFLOP/s, the FP64 matrix peak AMD publishes for the MI355X.  Before timing, two calls must return
equal bytes.  bh_depthcov_sets is timed on the same rows beside it: the yardstick.

Leg (b): StationPool.data_covariance() in one pass -- forward pass, scans and contraction -- on one finished pool of 4
stations x 8 chains whose sample arrays are tiled to 64 stations, against numpy on the same rows on one host core: the
interpolation of every row onto the grid and the weighted cross-covariance per station, GIVEN the modelled data (the host
has no forward pass to time; the device's matrix is pulled once, outside the timing).  First the covariances must agree
to 1e-9 of the standard deviations' scale.
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
from bayhunter_amd import _lib, covariance as cov, convergence as conv, datacov as dc, datafits as df, selection as sel  # noqa: E402
from depthcov_bench import NDEP, PEAK_FP64_MATRIX, make_rows  # noqa: E402

NDATA = 222


def timed(fn, repeats, sync):
    ts = []
    for _ in range(max(5, repeats)):
        sync()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(seconds_median=float(np.median(ts)), seconds_min=min(ts), seconds_max=max(ts), repeats=len(ts))


def kernel_leg(args, lines):
    import torch
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    dep = np.linspace(0, 100, NDEP)
    K, S, R = NDEP + 1, NDATA, 1000000
    npairs = -(-K // 16) * -(-S // 16)
    rows, w, extra = make_rows(R, dev)
    g = torch.Generator(device=dev).manual_seed(2)
    Y = torch.rand((R, S), generator=g, device=dev, dtype=torch.float64) + rows[:, :1].to(torch.float64)
    err = (torch.rand((R, 1), generator=g, device=dev) < 0.01).to(torch.int32)
    sync = lambda: torch.cuda.synchronize(dev)
    for Z in (1, 256):
        start = (np.arange(Z + 1, dtype=np.int64) * R) // Z
        cx, cy = np.tile(np.r_[np.full(NDEP, 3.5), 1.75], (Z, 1)), np.full((Z, S), 4.)
        call = lambda: dc.datacov_sets(rows, w, extra, Y, S, err, start, dep, cx, cy, stream)
        a, b = call(), call()
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
        assert int(a['total'].sum() + a['excluded'].sum()) == int(w.sum()) and a['excluded'].sum() > 0
        blocks = int(np.sum(-(-np.diff(start) // _lib.DEPTHCOV_BLOCK_ROWS)))
        flops = 2048. * npairs * sum(-(-min(_lib.DEPTHCOV_BLOCK_ROWS, int(n) - b0) // 4) for n in np.diff(start)
                                     for b0 in range(0, int(n), _lib.DEPTHCOV_BLOCK_ROWS))
        line = dict(leg='datacov', rows=R, sets=Z, K=K, S=S, tile_pairs=npairs, blocks=blocks, mfma_flops=flops,
                    result_bytes=Z * K * S * 8, src=_lib.loaded_hash())
        line.update(timed(call, args.repeats, sync))
        line.update(tflops=flops / line['seconds_median'] / 1e12,
                    share_of_fp64_matrix_peak=flops / line['seconds_median'] / PEAK_FP64_MATRIX)
        yard = timed(lambda: cov.depthcov_sets(rows, w, extra, start, dep, cx, stream), args.repeats, sync)
        line.update({'depthcov_' + k: v for k, v in yard.items()})
        lines.append(line)
        print(json.dumps(line), flush=True)


def host_cross(X, Y, w):
    """The weighted population cross-covariance of the columns of X and Y, as np.cov(..., fweights=w, bias=True) forms
    its own: centred on the weighted means, one matrix product."""
    W = w.sum()
    dx, dy = X - (w @ X) / W, Y - (w @ Y) / W
    return (dx * w[:, None]).T @ dy / W


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
    kw = dict(extras=('vpvs',), dev=1e9, strict=False)
    Z = 64
    tiled = Tiled(spool, Z)
    tiled.stations, tiled.per_station = [stations[s % 4] for s in range(Z)], ()
    one = dc.stations_data_covariance(tiled, **kw)
    inner, c = tiled.pool, tiled.chains_per_station
    ci, ri, w, set_start, _ = sel.station_rows(inner, c, 'weighted', 1e9, True)
    vpvs = inner.vpvs[ci, ri].astype(np.float64)
    _, Yd, err, _ = df.forward_matrix(stations[0], inner.models[ci, ri], vpvs, inner.priors.get('mantle'))
    S = one.mean_y.shape[1]
    Y = Yd[:, :S].cpu().numpy()
    ok = ~(err.cpu().numpy() != 0).any(axis=1) & ~np.isnan(Y).any(axis=1)
    del Yd, err

    def host():
        out = []
        for z in range(Z):
            a, b = int(set_start[z]), int(set_start[z + 1])
            k = ok[a:b]
            X = np.column_stack((conv.vs_at(inner.models[ci[a:b], ri[a:b]], dep), vpvs[a:b]))
            out.append(host_cross(X[k], Y[a:b][k], w[a:b][k].astype(np.float64)))
        return out
    for z, want in enumerate(host()):
        scale = np.outer(one.std_x[z], one.std_y[z]).max()
        assert np.abs(one.cov[z] - want).max() <= 1e-9 * scale, z
    line = dict(leg='stations', stations=Z, chains=8, iter_main=args.main, K=NDEP + 1, S=S, rows=int(ci.size),
                models=int(one.nmodels.sum()), excluded=int(one.nexcluded.sum()), host_processes=1, src=_lib.loaded_hash())
    for name, fn in (('one_pass', lambda: dc.stations_data_covariance(tiled, **kw)), ('host_given_data', host)):
        line.update({name + '_' + k: v for k, v in timed(fn, args.repeats, torch.cuda.synchronize).items()})
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
