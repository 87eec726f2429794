"""Timing of the velocity-depth posterior (bayhunter_amd.posterior.summarize) against the numpy restatement.

    python tools/posterior_bench.py [--rows 2000000] [--wmax 9] [--depths 61] [--host-rows 20000] [--out FILE]

Random 1..20-nucleus models (float32, the pool's storage type) with weights 1..wmax.  Reports seconds and
weighted rows/s of: summarize on rows already on the device (every pass incl. the host hand-overs between
them), summarize from host arrays (H2D included), and the test restatement (tests/posterior_ref.py, one
core) on --host-rows rows.  One JSON line, stamped with the library's source hash.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_rows(rs, R, maxn=21):
    n = rs.randint(1, maxn, R)
    k = np.arange(maxn)[None, :]
    rows = np.full((R, 2 * maxn), np.nan, dtype=np.float32)
    vs = rs.uniform(2, 5, (R, maxn)).astype(np.float32)
    z = np.sort(rs.uniform(0, 60, (R, maxn)).astype(np.float32), axis=1)
    z = np.where(k < n[:, None], z, np.inf)
    z.sort(axis=1)
    have = k < n[:, None]
    rows[:, :maxn][have] = vs[have]
    r, c = np.nonzero(have)
    rows[r, n[r] + c] = z[r, c]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2000000)
    ap.add_argument('--wmax', type=int, default=9)
    ap.add_argument('--depths', type=int, default=61)
    ap.add_argument('--host-rows', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import bayhunter_amd
    from bayhunter_amd import _lib
    from bayhunter_amd.posterior import summarize
    bayhunter_amd.build()
    rs = np.random.RandomState(1)
    rows = make_rows(rs, a.rows)
    w = rs.randint(1, a.wmax + 1, a.rows).astype(np.int32)
    W = int(w.sum())
    dep = np.linspace(0, 60, a.depths)
    drows, dw = torch.from_numpy(rows).cuda(), torch.from_numpy(w).cuda()
    summarize(drows, dw, dep_int=dep)                      # warm-up (module load, allocation)
    torch.cuda.synchronize()
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        summarize(drows, dw, dep_int=dep)
        t.append(time.perf_counter() - t0)
    dev_s = min(t)
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        summarize(rows, w, dep_int=dep)
        t.append(time.perf_counter() - t0)
    e2e_s = min(t)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import posterior_ref as ref
    hr = min(a.host_rows, a.rows)
    t0 = time.perf_counter()
    ref.summarize(rows[:hr], w[:hr], dep)
    host_s = time.perf_counter() - t0
    Wh = int(w[:hr].sum())
    rec = dict(tool='posterior_bench', src=_lib.loaded_hash(), rows=a.rows, weighted_rows=W, depths=a.depths,
               device_s=round(dev_s, 5), device_weighted_rows_per_s=W / dev_s,
               end_to_end_s=round(e2e_s, 5), end_to_end_weighted_rows_per_s=W / e2e_s,
               host_rows=hr, host_weighted_rows=Wh, host_s=round(host_s, 4), host_weighted_rows_per_s=Wh / host_s,
               speedup_device_vs_host=(W / dev_s) / (Wh / host_s), gpu=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
