#!/bin/bash
# this tree against the checkout under _ab_old/ (git worktree of an earlier commit that has bench.py --full, built), the full bench line of
# both on ONE box; the lines go to $OUT (default results/)
cd ${GRAFT_REPO_ROOT:-.}
OUT=$(mkdir -p "${OUT:-results}" && cd "${OUT:-results}" && pwd)
for i in 1 2; do
  (cd _ab_old && timeout -k 10 500 python3 bench.py --full --cpu-baseline-samples 0 2>/dev/null > "$OUT/ab_round_old_$i.json") || exit 1
  timeout -k 10 500 python3 bench.py --full --cpu-baseline-samples 0 2>/dev/null > "$OUT/ab_round_new_$i.json" || exit 1
done
OUT="$OUT" python3 - <<'PY'
import json, os
for n in ("old_1", "new_1", "old_2", "new_2"):
    d = json.loads(open(os.path.join(os.environ["OUT"], f"ab_round_{n}.json")).read().strip().splitlines()[-1])
    print(n, "cfg2", d["value"], [(e["config"]["workload"][:14], e["value"]) for e in d["extra"]])
PY
