"""What the Rayleigh-wave ellipticity costs (ell_kernel, bayhunter_amd/csrc/ellipticity.hip), one process, every leg
warmed once and the median of --repeats (default 7) device-synchronised wall times reported; one JSON line per size.

Per batch size (default 524 288 and 1 024 ten-layer models of bayhunter_amd.synthetic.draw_models, 21 periods):

  forward_s      ForwardEngine(swd=[rdispph]).run: the search alone
  with_ell_s     ForwardEngine(swd=[rdispph], ell=[rellip]).run on the same models: the search and the pass behind it
  increment_s    with_ell_s - forward_s, and increment_pct of forward_s
  ell_alone_s    bh_ell_batch alone on the phase velocities the search left in HBM

    python tools/ellipticity_bench.py [--sizes 524288 1024] [--layers 10] [--nper 21] [--repeats 7] [--out FILE]

Two more modes, one JSON line each, appended to profiles/ellipticity_plan.jsonl (or --out) and stamped with the hash of
the loaded library:

  --plan   the ellipticity stage of the evaluation plan: bh_eval_submit -> bh_eval_wait of a plan for rdispph + prf +
           rellip against the same plan without rellip, and rdispph + rellip against rdispph, at 4 096 and 65 536
           ten-layer rows (--plan-sizes)
  --rows   ell_rows_kernel alone (bh_ell_batch_rows without and with the dispersion launch's processing order) against
           ell_kernel alone (bh_ell_batch), on a ragged batch of 2-14 layers and on a ten-layer batch, at 524 288 and
           1 024 models (--sizes); medians, and the fastest and slowest of the repeats
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
    ap.add_argument('--plan', action='store_true')
    ap.add_argument('--rows', action='store_true')
    ap.add_argument('--plan-sizes', nargs='*', type=int, default=[4096, 65536])
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

    def spread(secs):
        return dict(median_s=round(float(np.median(secs)), 6), min_s=round(min(secs), 6), max_s=round(max(secs), 6))

    def emit(d):
        d.update(tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats, nper=args.nper)
        line = json.dumps(d)
        print(line, flush=True)
        out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                       'ellipticity_plan.jsonl')
        with open(out, 'a') as fh:
            fh.write(line + '\n')

    if args.plan:
        from bayhunter_amd import targets as T
        t = np.linspace(-5, 35, 201)

        def joint_of(refs):
            made = {'rdispph': lambda: T.RayleighDispersionPhase(per, np.full(args.nper, 3.5)),
                    'prf': lambda: T.PReceiverFunction(t, np.zeros(201)),
                    'rellip': lambda: T.RayleighEllipticity(per, np.full(args.nper, 0.8))}
            joint = T.JointTarget([made[r]() for r in refs])
            # the tutorial's noise models: diagonal for the period targets, dense Gaussian (r = 0.9) for the receiver function
            joint.set_target_covariance([True] * len(refs), [0.9 if r == 'prf' else 0.0 for r in refs], 1e-5)
            return joint

        def plan_seconds(refs, B, H, VP, VS, RHO, nl):
            joint = joint_of(refs)
            with joint.eval_plan(B, args.layers) as plan:
                plan.packed[:, 0], plan.packed[:, 1], plan.packed[:, 2], plan.packed[:, 3] = H, VP, VS, RHO
                plan.nlay[:] = nl
                plan.noise[:, 0::2], plan.noise[:, 1::2] = 0.0, 0.02

                def once():
                    plan.submit(B)
                    plan.wait()
                secs = median_of(once)[1]
                refused = int((plan.wait()[0] == -1e15).sum())
            return secs, refused
        res = []
        for B in args.plan_sizes:
            H, VP, VS, RHO, nl = draw_models(B, args.layers, seed=1)
            for base in (('rdispph', 'prf'), ('rdispph',)):
                s0, r0 = plan_seconds(base, B, H, VP, VS, RHO, nl)
                s1, r1 = plan_seconds(base + ('rellip',), B, H, VP, VS, RHO, nl)
                m0, m1 = float(np.median(s0)), float(np.median(s1))
                res.append(dict(models=B, layers=args.layers, base='+'.join(base), base_plan=spread(s0), with_ell_plan=spread(s1),
                                increment_s=round(m1 - m0, 6), increment_pct=round(100 * (m1 - m0) / m0, 2),
                                refused_base=r0, refused_with_ell=r1))
        emit(dict(bench='ellipticity_plan', results=res))
    if args.rows:
        import ctypes as C
        res = []
        for B in args.sizes:
            for name, layers in (('ragged_2_14', (2, 14)), ('layers_%d' % args.layers, args.layers)):
                H, VP, VS, RHO, nl = draw_models(B, layers, seed=1)
                plain = ForwardEngine(swd=[SwdSpec('rdispph', per)])
                models = plain.upload(H, VP, VS, RHO, nl)
                out0, err0 = plain.run(models)
                L = models.Lmax
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                keys = torch.empty(B, dtype=torch.int32, device=out0.device)
                _lib.check(lib.bh_swd_order_keys(B, L, 4 * L, models.nlay.data_ptr(), models.H.data_ptr(), models.VS.data_ptr(),
                                                 float(per.max()), 1, keys.data_ptr(), st))
                order = torch.argsort(keys).to(torch.int32)
                ell = [torch.empty((B, args.nper), dtype=torch.float64, device=out0.device) for _ in range(3)]
                head = (B, L, 4 * L, models.nlay.data_ptr(), models.H.data_ptr(), models.VP.data_ptr(), models.VS.data_ptr(),
                        models.RHO.data_ptr(), args.nper, plain.periods.data_ptr(), 0, out0.data_ptr(), plain.row,
                        err0.data_ptr(), 1, 1)
                dense = median_of(lambda: _lib.check(lib.bh_ell_batch(*(head + (ell[0].data_ptr(), args.nper, st)))))[1]
                rows = median_of(lambda: _lib.check(lib.bh_ell_batch_rows(
                    *(head + (ell[1].data_ptr(), args.nper, None, 0, st)))))[1]
                ordered = median_of(lambda: _lib.check(lib.bh_ell_batch_rows(
                    *(head + (ell[2].data_ptr(), args.nper, order.data_ptr(), 0, st)))))[1]
                for e in ell[1:]:
                    assert torch.equal(torch.nan_to_num(e, nan=-1.0), torch.nan_to_num(ell[0], nan=-1.0))
                md = float(np.median(dense))
                res.append(dict(models=B, batch=name, ell_kernel=spread(dense), ell_rows_kernel=spread(rows),
                                ell_rows_kernel_ordered=spread(ordered),
                                rows_vs_dense_pct=round(100 * (float(np.median(rows)) - md) / md, 2),
                                ordered_vs_dense_pct=round(100 * (float(np.median(ordered)) - md) / md, 2)))
        emit(dict(bench='ellipticity_rows', results=res))
    if args.plan or args.rows:
        return

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
