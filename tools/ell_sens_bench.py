"""What the ellipticity sensitivity kernels cost (bh_ell_sens_batch with K_phase: ell_sens_root_kernel + ell_sens_kernel,
bayhunter_amd/csrc/ell_sens.hip) against the phase-velocity pass (bh_sens_batch, Rayleigh) on the same rows: one process,
every leg warmed once, the median of --repeats (default 7) device-synchronised wall times; one JSON line per size,
appended to profiles/ell_sens_bench.jsonl (or --out) and stamped with the hash of the loaded library.

Per batch size (default 1 and 65 536 ten-layer models of bayhunter_amd.synthetic.draw_models, 21 periods):

  phase_s            ForwardEngine.sensitivity (bh_sens_batch) on the phase velocities the search left in HBM
  ell_s              ForwardEngine.ell_sensitivity (bh_ell_sens_batch, K_phase written too) on the same
  ell_over_phase     ell_s / phase_s.  The passes per lane are the phase pass's, plus one per (model, period) at the
                     polished root; what grows is the arithmetic per pass (G beside F) and a second K written

NOT measured here: the two kernels of either call apart, the call without K_phase, other layer counts than --layers,
ragged batches, and the pass inside summarize().

    python tools/ell_sens_bench.py [--sizes 1 65536] [--layers 10] [--nper 21] [--repeats 7] [--out FILE]
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
    from bayhunter_amd.engine import EllSpec, ForwardEngine, SwdSpec
    from bayhunter_amd.synthetic import draw_models
    per = np.linspace(1, 41, args.nper)
    out_path = args.out or os.path.join(root, 'profiles', 'ell_sens_bench.jsonl')

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
        # the ellipticity target shares the phase target: both passes read the same columns
        eng = ForwardEngine(swd=[SwdSpec('rdispph', per)], ell=[EllSpec('rellip', per, 0, True)])
        models = eng.upload(H, VP, VS, RHO, nl)
        out, err = eng.run(models)
        phase = median_of(lambda: eng.sensitivity(models, out=out, err=err))
        ell = median_of(lambda: eng.ell_sensitivity(models, out=out, err=err))
        a, b = eng.sensitivity(models, out=out, err=err), eng.ell_sensitivity(models, out=out, err=err)
        torch.cuda.synchronize()
        valued = torch.isfinite(b['K']).all(dim=(1, 2, 3))
        same = bool(torch.equal(torch.nan_to_num(a['K'][valued]), torch.nan_to_num(b['K_phase'][valued])))
        mp, me = float(np.median(phase)), float(np.median(ell))
        d = dict(bench='ell_sens', wave='rayleigh', models=B, layers=args.layers, nper=args.nper, phase_s=round(mp, 6),
                 ell_s=round(me, 6), ell_over_phase=round(me / mp, 3), ell_ns_per_model_period=round(1e9 * me / (B * args.nper), 1),
                 phase_all_s=[round(x, 6) for x in phase], ell_all_s=[round(x, 6) for x in ell],
                 valued=int(valued.sum().item()), phase_valued=int(torch.isfinite(a['K']).all(dim=(1, 2, 3)).sum().item()),
                 k_phase_is_the_phase_pass=same,
                 not_measured=['the two kernels apart', 'without K_phase', 'other layer counts', 'ragged batches',
                               'inside summarize()'],
                 tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats)
        line = json.dumps(d)
        print(line, flush=True)
        with open(out_path, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
