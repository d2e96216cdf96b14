#!/bin/bash
# round-end check on one box:  tools/gpu_final.sh bench  (smoke + the full bench line)   |   tools/gpu_final.sh tests  (the whole GPU suite)
# logs and the bench line go to $OUT (default results/)
cd ${GRAFT_REPO_ROOT:-.}
OUT=${OUT:-results}; mkdir -p "$OUT"
if [ "$1" = "bench" ]; then
  timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > "$OUT/final_smoke.log" 2>&1 || { tail -5 "$OUT/final_smoke.log"; exit 1; }
  timeout -k 10 800 python bench.py --full > "$OUT/final_bench_line.json" 2> "$OUT/final_bench_line.err" || { tail -5 "$OUT/final_bench_line.err"; exit 1; }
  echo "bench done"
else
  timeout -k 10 1150 python -m pytest tests -x -q -m gpu > "$OUT/final_gpu_tests.log" 2>&1; rc=$?
  tail -5 "$OUT/final_gpu_tests.log"
  exit $rc
fi
