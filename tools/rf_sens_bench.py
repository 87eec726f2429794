"""What the receiver-function sensitivity kernels cost (bh_rf_sens_batch: rf_sens_kernel, bayhunter_amd/csrc/rf_sens.hip)
against the forward trace (bh_rf_batch: rf_kernel) on the same rows: one process, every leg warmed once, the median of
--repeats (default 7) device-synchronised wall times; one JSON line per size, appended to profiles/rf_sens_bench.jsonl
(or --out) and stamped with the hash of the loaded library.

Per batch size (default 1, 1 024 and 65 536 ten-layer models of bayhunter_amd.synthetic.draw_models; nsamp 256, all
samples written):

  forward_s          bh_rf_batch on the rows
  sens_s             bh_rf_sens_batch on the same rows, without the optional rf output
  sens_over_forward  sens_s / forward_s.  The pass runs the forward phases 2 (4 L - 1) times per model -- 78 at ten
                     layers -- minus the global write of the traces: `expected` in the line
  traces_per_s       2 (4 L - 1) B / sens_s, beside the forward launch's B / forward_s

NOT measured here: other layer counts than --layers and other lengths than --nsamp, hardware counters, the paired and the
sequential LDS regime apart (nsamp 256 takes the paired form), ragged batches, the call with the rf output.

    python tools/rf_sens_bench.py [--sizes 1 1024 65536] [--layers 10] [--nsamp 256] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='*', type=int, default=[1, 1024, 65536])
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--nsamp', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    from bayhunter_amd import _lib
    from bayhunter_amd.synthetic import draw_models
    lib = _lib.load()
    dev = torch.device('cuda')
    out_path = args.out or os.path.join(root, 'profiles', 'rf_sens_bench.jsonl')
    n, L = args.nsamp, args.layers
    par = _lib.RfParams(6.4, 1.0, 5.0, 5.0, -1.0, n, 0, n, 0)

    def median_of(fn):
        def timed():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        timed()                                              # warm
        return [timed() for _ in range(args.repeats)]

    for B in args.sizes:
        H, VP, VS, RHO, nl = draw_models(B, L, seed=1)
        d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev) for x in (H, VP, VS, RHO)]
        dn = torch.from_numpy(np.asarray(nl, dtype=np.int32)).to(dev)
        out = torch.empty((B, n), dtype=torch.float64, device=dev)
        K = torch.empty((B, n, 4, L), dtype=torch.float64, device=dev)
        head = (B, L, L, dn.data_ptr()) + tuple(x.data_ptr() for x in d) + (None, None, C.byref(par))
        fwd = median_of(lambda: _lib.check(lib.bh_rf_batch(*head, out.data_ptr(), n, None, 0, None)))
        sens = median_of(lambda: _lib.check(lib.bh_rf_sens_batch(*head, K.data_ptr(), n * 4 * L, None, 0, None, 0, None)))
        mf, ms = float(np.median(fwd)), float(np.median(sens))
        traces = 2 * (4 * L - 1)
        line = json.dumps(dict(
            bench='rf_sens', models=B, layers=L, nsamp=n, forward_s=round(mf, 6), sens_s=round(ms, 6),
            sens_over_forward=round(ms / mf, 2), expected=traces, forward_traces_per_s=round(B / mf, 1),
            sens_traces_per_s=round(traces * B / ms, 1), forward_all_s=[round(x, 6) for x in fwd],
            sens_all_s=[round(x, 6) for x in sens], finite=bool(torch.isfinite(K).all().item()),
            not_measured=['other layer counts and lengths', 'hardware counters', 'the paired and the sequential LDS regime apart',
                          'ragged batches', 'with the rf output'],
            tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats))
        print(line, flush=True)
        with open(out_path, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
