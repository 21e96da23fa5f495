#!/bin/bash
# usage: runbench.sh <label> [outdir]   (on an MI355X, from the repository root; outdir defaults to bench_out)
out=${2:-bench_out}; mkdir -p "$out"
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $out/gpu_tests.log 2>&1; rc=$?; tail -1 $out/gpu_tests.log; [ $rc -eq 0 ] || exit $rc
for n in 1 2; do timeout -k 10 300 python bench.py --full --steps 600 --warmup 60 --no-cpu-baseline --inflight $n > $out/dbgx.log 2>&1 || { rc=$?; tail -5 $out/dbgx.log; exit $rc; }; python - <<PY
import json
try:
    d=json.loads(open("$out/dbgx.log").read().strip().splitlines()[-1]); print("$1 inflight", $n, round(d["ms_per_step"]*1e3,1), d["config"]["matches_distinct"], {k:(round(v["avg_launch_us"],1), v["launches"]) for k,v in d["kernels"].items()})
except Exception as e: print("FAIL", open("$out/dbgx.log").read()[-300:])
PY
done
