"""What the posterior receiver-function sensitivity reduction costs (csrc/rf_sens_sets.hip), one process, every leg warmed
once, the median of --repeats (default 7) device-synchronised wall times reported with every run; one JSON line per leg,
appended to profiles/rf_sens_sets.jsonl and stamped with the hash of the loaded library.  On --rows (default 65 536)
ten-layer models of bayhunter_amd.synthetic.draw_models, a trace of --samples (default 256) samples, --bins (default 100)
depth bins, kind 'vs_total', integer weights:

  (a) the reduction alone: bh_rf_sens_sets_create + add + finish with its copies to the host, as 1 set and as 256 sets;
  (b) the bh_rf_sens_batch call that made K for the same rows;
  (c) the same numbers by the route that existed before: the same K through bh_sens_sets_* in slices of at most 60
      samples with a dummy finite c_out -- bh_sens_sets_add takes no row stride, so every slice of K is first copied into
      rows of its own, and that copy is part of the route (it is also reported alone).

Each leg is a run of its own (--legs a | b | c), so that a caller can give every step its own time limit:

    timeout -k 10 300 python tools/rf_sens_sets_bench.py --legs b
    python tools/rf_sens_sets_bench.py [--legs a,b,c] [--rows 65536] [--samples 256] [--bins 100] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='a,b,c')
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--bins', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=os.path.join(here, 'profiles', 'rf_sens_sets.jsonl'))
    args = ap.parse_args()
    sys.path.insert(0, here)
    import torch
    from bayhunter_amd import _lib, sensitivity as sens
    from bayhunter_amd.engine import ForwardEngine, RfSpec
    from bayhunter_amd.synthetic import draw_models
    legs = args.legs.split(',')

    def emit(d):
        d = dict(d, tag=args.tag, src=_lib.loaded_hash(), repeats=args.repeats, device=torch.cuda.get_device_name(0),
                 rows=args.rows, layers=args.layers, samples=args.samples, bins=args.bins, kind='vs_total')
        line = json.dumps(d)
        print(line, flush=True)
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def runs_of(fn):
        timed(fn)                                            # warm
        secs = [timed(fn)[0] for _ in range(args.repeats)]
        return dict(median_s=round(float(np.median(secs)), 6), min_s=round(min(secs), 6), max_s=round(max(secs), 6),
                    runs_s=[round(x, 6) for x in secs])

    B, nt = args.rows, args.samples
    edges = np.linspace(0., 100., args.bins + 1)
    H, VP, VS, RHO, nl = draw_models(B, args.layers, seed=1)
    eng = ForwardEngine(rf=[RfSpec('prf', np.arange(nt) * 0.2 - 5., 1.0, 6.4)])
    models = eng.upload(H, VP, VS, RHO, nl)
    res = eng.rf_sensitivity(models)
    q = (models.VP / models.VS).contiguous()
    w = torch.from_numpy(np.random.RandomState(2).randint(0, 300, B).astype(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    code = _lib.SENS_KINDS['vs_total']
    torch.cuda.synchronize()

    if 'b' in legs:
        emit(dict(bench='rf_sens_batch', rf_sens_batch=runs_of(lambda: eng.rf_sensitivity(models))))

    if 'a' in legs:
        for nsets in (1, 256):
            start = np.linspace(0, B, nsets + 1).astype(np.int64)

            def reduce():
                with sens.RfSensSets(start, nt, np.arange(nt), edges, code, 0.32, stream) as hd:
                    hd.add(0, models, res['K'], res['rf'], q, w)
                    return hd.finish()
            r = runs_of(reduce)
            sums = reduce()
            emit(dict(bench='rf_sens_sets_reduction', sets=nsets, reduction=r, rows_per_s=round(B / r['median_s']),
                      weight_total=int(sums['total'].sum()), weight_excluded=int(sums['excluded'].sum()),
                      not_measured=['other layer counts, sample counts and bin counts', 'a selection of the samples',
                                    'sets cut over several add calls', 'other kinds than vs_total',
                                    'the pool-level calls (ChainPool.rf_sensitivity, StationPool.rf_sensitivity)']))

    if 'c' in legs:
        c_out = torch.full((B, _lib.MAX_PERIODS), 3.0, dtype=torch.float64, device=w.device)
        slices = [(s, min(nt, s + _lib.MAX_PERIODS)) for s in range(0, nt, _lib.MAX_PERIODS)]
        copy = runs_of(lambda: [res['K'][:, a:b].contiguous() for a, b in slices][-1])
        for nsets in (1, 256):
            start = np.linspace(0, B, nsets + 1).astype(np.int64)

            def sliced():
                out = []
                for a, b in slices:
                    Ks = res['K'][:, a:b].contiguous()
                    with sens.SensSets(start, b - a, edges, code, 0.32, stream) as hd:
                        hd.add(0, models, Ks, c_out[:, :b - a].contiguous(), q, w)
                        out.append(hd.finish())
                return out
            emit(dict(bench='sens_sets_in_slices', sets=nsets, slices=len(slices), sliced=runs_of(sliced), copy_of_K_alone=copy))


if __name__ == '__main__':
    main()
