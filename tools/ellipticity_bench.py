"""What the Rayleigh-wave ellipticity costs (ell_kernel, bayhunter_amd/csrc/ellipticity.hip), one process, every leg
warmed once and the median of --repeats (default 7) device-synchronised wall times reported; one JSON line per size.

Per batch size (default 524 288 and 1 024 ten-layer models of bayhunter_amd.synthetic.draw_models, 21 periods):

  forward_s      ForwardEngine(swd=[rdispph]).run: the search alone
  with_ell_s     ForwardEngine(swd=[rdispph], ell=[rellip]).run on the same models: the search and the pass behind it
  increment_s    with_ell_s - forward_s, and increment_pct of forward_s
  ell_alone_s    bh_ell_batch alone on the phase velocities the search left in HBM

    python tools/ellipticity_bench.py [--sizes 524288 1024] [--layers 10] [--nper 21] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='*', type=int, default=[524288, 1024])
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--nper', type=int, default=21)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from bayhunter_amd import _lib
    from bayhunter_amd.engine import EllSpec, ForwardEngine, SwdSpec
    from bayhunter_amd.synthetic import draw_models
    lib = _lib.load()
    per = np.linspace(1, 41, args.nper)

    def median_of(fn):
        def timed():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        timed()                                              # warm
        secs = [timed() for _ in range(args.repeats)]
        return float(np.median(secs)), secs

    for B in args.sizes:
        H, VP, VS, RHO, nl = draw_models(B, args.layers, seed=1)
        plain = ForwardEngine(swd=[SwdSpec('rdispph', per)])
        both = ForwardEngine(swd=[SwdSpec('rdispph', per)], ell=[EllSpec('rellip', per)])
        models = plain.upload(H, VP, VS, RHO, nl)
        out0, err0 = plain.alloc_out(B)
        out1, err1 = both.alloc_out(B)
        fwd_s, fwd_all = median_of(lambda: plain.run(models, out=out0, err=err0))
        both_s, both_all = median_of(lambda: both.run(models, out=out1, err=err1))
        assert torch.equal(out0[:, :args.nper], out1[:, :args.nper])
        ell = torch.empty((B, args.nper), dtype=torch.float64, device=out0.device)
        L = models.Lmax

        def alone():
            _lib.check(lib.bh_ell_batch(B, L, 4 * L, models.nlay.data_ptr(), models.H.data_ptr(), models.VP.data_ptr(),
                                        models.VS.data_ptr(), models.RHO.data_ptr(), args.nper, plain.periods.data_ptr(), 0,
                                        out0.data_ptr(), plain.row, err0.data_ptr(), 1, 1, ell.data_ptr(), args.nper,
                                        torch.cuda.current_stream().cuda_stream))
        alone_s, alone_all = median_of(alone)
        assert torch.equal(torch.nan_to_num(ell, nan=-1.0), torch.nan_to_num(out1[:, args.nper:2 * args.nper], nan=-1.0))
        d = dict(bench='ellipticity', models=B, layers=args.layers, nper=args.nper, forward_s=round(fwd_s, 6),
                 with_ell_s=round(both_s, 6), increment_s=round(both_s - fwd_s, 6),
                 increment_pct=round(100 * (both_s - fwd_s) / fwd_s, 2), ell_alone_s=round(alone_s, 6),
                 ell_alone_pct_of_forward=round(100 * alone_s / fwd_s, 2),
                 ell_alone_ns_per_model_period=round(1e9 * alone_s / (B * args.nper), 3),
                 forward_all_s=[round(x, 6) for x in fwd_all], with_ell_all_s=[round(x, 6) for x in both_all],
                 ell_alone_all_s=[round(x, 6) for x in alone_all], solved=int((err0[:, 0] == 0).sum().item()),
                 tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats)
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
