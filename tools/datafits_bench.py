"""Timing of the modelled-data statistics (bayhunter_amd.datafits.summarize): forward pass against statistics.

    python tools/datafits_bench.py [--rows 100000 1000000] [--wmax 9] [--reps 3] [--out FILE]

The joint10 layout (Rayleigh phase velocity, 21 periods, and a P receiver function, 201 samples): random
2..10-nucleus models with weights 1..wmax.  Per size: the forward pass into one device matrix
(datafits.forward_matrix: layers_from_voronoi + ForwardEngine.run) and the statistics on it (one bh_datafits
handle: mask, scan, finish with the default percentiles, the median and a 100-bin histogram per sample), each
synchronised, best of --reps.  One JSON line, stamped with the library's source hash.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_rows(rs, R, maxn=10):
    n = rs.randint(2, maxn + 1, R)
    k = np.arange(maxn)[None, :]
    rows = np.full((R, 2 * maxn), np.nan)
    vs = rs.uniform(2, 5, (R, maxn))
    z = np.sort(np.where(k < n[:, None], rs.uniform(0, 60, (R, maxn)), np.inf), axis=1)
    have = k < n[:, None]
    rows[:, :maxn][have] = vs[have]
    r, c = np.nonzero(have)
    rows[r, n[r] + c] = z[r, c]
    return rows, rs.uniform(1.6, 1.9, R)


def joint10(rs):
    from bayhunter_amd import targets as T
    per, trf = np.linspace(1, 41, 21), np.linspace(-5, 35, 201)
    joint = T.JointTarget([T.RayleighDispersionPhase(per, rs.normal(3.5, .2, per.size)),
                           T.PReceiverFunction(trf, rs.normal(0, .05, trf.size))])
    joint.set_target_covariance([True, True], [0.0, 0.0])
    return joint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--wmax', type=int, default=9)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import bayhunter_amd
    from bayhunter_amd import _lib
    from bayhunter_amd.datafits import DEFAULT_Q, Fits, forward_matrix, percentile_ranks, summarize
    bayhunter_amd.build()
    rs = np.random.RandomState(1)
    joint = joint10(rs)
    rec = dict(tool='datafits_bench', src=_lib.loaded_hash(), layout='joint10 (rdispph 21 + prf 201)',
               gpu=torch.cuda.get_device_name(0), sizes=[])
    for R in a.rows:
        rows, vpvs = make_rows(rs, R)
        w = rs.randint(1, a.wmax + 1, R).astype(np.int32)
        drows, dv, dw = (torch.from_numpy(x).cuda() for x in (rows, vpvs, w))
        summarize(joint, drows[:1000], dv[:1000], dw[:1000])           # warm-up (module load, allocation)
        torch.cuda.synchronize()
        tf, ts = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng, Y, err, bl = forward_matrix(joint, drows, dv)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            st = torch.cuda.current_stream().cuda_stream
            f = Fits(Y, eng.ncols, dw, err, st)
            s = f.scan()
            virt, lo, hi = percentile_ranks(DEFAULT_Q, s['total'])
            ranks = np.unique(np.r_[lo, hi, (s['total'] - 1) // 2, s['total'] // 2])
            edges = np.stack([np.linspace(s['vmin'][:21].min(), s['vmax'][:21].max(), 101),
                              np.linspace(s['vmin'][21:].min(), s['vmax'][21:].max(), 101)])
            eset = np.r_[np.zeros(21), np.ones(eng.ncols - 21)].astype(np.int32)
            f.finish(ranks, edges, eset)
            f.close()
            t2 = time.perf_counter()
            tf.append(t1 - t0)
            ts.append(t2 - t1)
            del Y, err
        t0 = time.perf_counter()
        res = summarize(joint, drows, dv, dw)
        torch.cuda.synchronize()
        tot = time.perf_counter() - t0
        fwd, stat = min(tf), min(ts)
        rec['sizes'].append(dict(rows=R, weighted_rows=int(w.sum()), ncols=eng.ncols, ranks=int(ranks.size),
                                 nexcluded=res['nexcluded'], forward_s=round(fwd, 5), stats_s=round(stat, 5),
                                 stats_over_forward=round(stat / fwd, 4), summarize_s=round(tot, 5),
                                 forward_rows_per_s=R / fwd, matrix_gb=R * eng.row * 8 / 1e9,
                                 stats_gb_per_s_per_read=R * eng.row * 8 / 1e9 / stat))
        del drows, dv, dw
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
