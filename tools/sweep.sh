#!/bin/bash
# GPU-box helper: batch-size sweep of bench.py (no CPU baseline), one JSON line per batch size.
# usage: OUT=<results directory> tools/sweep.sh B ...
set -e
OUT=${OUT:?set OUT to the directory that takes the results}
mkdir -p "$OUT"
: > "$OUT/sweep.jsonl"
for B in "$@"; do
  timeout -k 10 200 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --batch $B >> "$OUT/sweep.jsonl" 2>> "$OUT/sweep.err"
done
OUT="$OUT" python - <<'PY'
import json, os
for l in open(os.path.join(os.environ['OUT'], 'sweep.jsonl')):
    r=json.loads(l)
    print(r['config']['models_per_gpu'], '%.3e evals/s'%r['value'], 'step %.2f ms'%r['ms_per_step'], 'swd %.2f ms rf %.2f ms'%(r['kernels_ms']['swd_kernel'], r['kernels_ms']['rf_kernel']), 'fp64 frac %.3f'%r['roofline']['frac'])
PY
