"""What the phase-velocity sensitivity kernels cost (sens_root_kernel + sens_kernel, bayhunter_amd/csrc/sensitivity.hip)
against the dispersion search alone: one process, every leg warmed once, the median of --repeats (default 7)
device-synchronised wall times; one JSON line per size, appended to profiles/sensitivity_bench.jsonl (or --out) and
stamped with the hash of the loaded library.

Per batch size (default 1 and 65 536 ten-layer models of bayhunter_amd.synthetic.draw_models, 21 periods) and wave type:

  search_s       ForwardEngine(swd=[rdispph | ldispph]).run: the search alone
  sens_s         bh_sens_batch (both kernels, one call) on the phase velocities the search left in HBM
  sens_over_search   sens_s / search_s

NOT measured here: the two kernels apart (they are launched by one call), other layer counts than --layers, ragged
batches, and the pass inside a sampler.

    python tools/sensitivity_bench.py [--sizes 1 65536] [--layers 10] [--nper 21] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='*', type=int, default=[1, 65536])
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--nper', type=int, default=21)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    from bayhunter_amd import _lib
    from bayhunter_amd.engine import ForwardEngine, SwdSpec
    from bayhunter_amd.synthetic import draw_models
    per = np.linspace(1, 41, args.nper)
    out_path = args.out or os.path.join(root, 'profiles', 'sensitivity_bench.jsonl')

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
        H, VP, VS, RHO, nl = draw_models(B, args.layers, seed=1)
        for wave, ref in (('rayleigh', 'rdispph'), ('love', 'ldispph')):
            eng = ForwardEngine(swd=[SwdSpec(ref, per)])
            models = eng.upload(H, VP, VS, RHO, nl)
            out, err = eng.alloc_out(B)
            search = median_of(lambda: eng.run(models, out=out, err=err))
            sens = median_of(lambda: eng.sensitivity(models, out=out, err=err))
            res = eng.sensitivity(models, out=out, err=err)
            torch.cuda.synchronize()
            solved = err[:, 0] == 0
            valued = torch.isfinite(res['K']).all(dim=(1, 2, 3))
            ms, mk = float(np.median(search)), float(np.median(sens))
            d = dict(bench='sensitivity', wave=wave, models=B, layers=args.layers, nper=args.nper, search_s=round(ms, 6),
                     sens_s=round(mk, 6), sens_over_search=round(mk / ms, 3),
                     sens_ns_per_model_period=round(1e9 * mk / (B * args.nper), 1),
                     search_all_s=[round(x, 6) for x in search], sens_all_s=[round(x, 6) for x in sens],
                     solved=int(solved.sum().item()), valued=int((valued & solved).sum().item()),
                     not_measured=['the two kernels apart', 'other layer counts', 'ragged batches', 'inside a sampler'],
                     tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats)
            line = json.dumps(d)
            print(line, flush=True)
            with open(out_path, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
