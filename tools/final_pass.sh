#!/bin/bash
# GPU-box helper: the end-of-round pass, in pieces that each fit one gpurun call (<= 20 min):
#   tools/final_pass.sh tests      GPU tests, smoke
#   tools/final_pass.sh profiles   rocprofv3 kernel trace + PMC passes: headline, cfg2, cfg3, cfg4, cfg5, 4096-chain pool
#   tools/final_pass.sh bench      bench line, two-rank rehearsal, one-rank RCCL line, chain pool sizes, phase profile
#   tools/final_pass.sh campaigns  random campaigns (kernel_fuzz, rf_fuzz)
# Outputs under $OUT (a directory the caller names); on the build host `python tools/summarize_profile.py <tag>` turns each profile into
# profiles/<tag>_{kernel_stats.csv,traffic.json,rocprofv3_summary.md} (stamped with the library's source hash).
set -e
cd "$(dirname "$0")/.."
R=${ROUND:-r04}
OUT=${OUT:?set OUT to the directory that takes the results}
mkdir -p "$OUT"
case "$1" in
tests)
    python -m pytest tests -m gpu -x -q > "$OUT/gpu_tests.log" 2>&1
    python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
    ;;
profiles)
    tools/profile.sh $R > "$OUT/profile_$R.log" 2>&1
    for w in cfg2 cfg3 cfg4 cfg5; do tools/profile.sh ${R}_$w --workload $w > "$OUT/profile_${R}_$w.log" 2>&1; done
    PROFILE_CMD="python3 $PWD/tools/chain_bench.py 4096" tools/profile.sh ${R}_pool4096 > "$OUT/profile_${R}_pool.log" 2>&1
    ;;
bench)
    python bench.py --full --steps 20 --warmup 5 > "$OUT/${R}_bench.json" 2> "$OUT/${R}_bench.err"
    BH_DIST_BACKEND=gloo python bench.py --full --gpus 2 --steps 5 --warmup 2 --no-configs > "$OUT/${R}_bench_n2_rehearsal.json" 2> "$OUT/${R}_bench_n2.err"
    BH_BENCH_FORCE_DIST=1 python bench.py --full --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-configs > "$OUT/${R}_bench_rccl1.json" 2> "$OUT/${R}_bench_rccl1.err"
    python tools/chain_bench.py 64 256 1024 4096 16384 65536 > "$OUT/${R}_chain_pool.jsonl" 2> "$OUT/chain_bench.err"
    python tools/host_phase_probe.py 256 1024 4096 16384 > "$OUT/${R}_host_phase_probe.jsonl" 2>/dev/null
    python tools/team_phase_profile.py > "$OUT/${R}_team_phase_profile.txt" 2>&1
    ( time python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err" ) 2> "$OUT/bench_default.time"
    ;;
campaigns)
    python tests/scenarios/kernel_fuzz.py 150 104 > "$OUT/${R}_kernel_fuzz.txt" 2>&1
    python tests/scenarios/rf_fuzz.py 60 91 > "$OUT/${R}_rf_fuzz.txt" 2>&1
    ;;
*)
    echo "usage: OUT=<results directory> tools/final_pass.sh tests|profiles|bench|campaigns"; exit 2 ;;
esac
