"""What runs beside AdamW: reads the per-dispatch CSV of a `rocprofv3 --kernel-trace` run of bench.py and prints, for the last
``--steps`` AdamW launches but one (steady state; the very last is the flush behind the timed region), the launch's interval and every
dispatch of ANOTHER queue (the CLIP tower's side stream) that starts or ends inside it.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 bench.py --steps 10 --warmup 3 ...
    python3 tools/adamw_overlap_report.py DIR [--steps 3]

"alone" is the shortest duration the trace holds for the same kernel at the same grid: an estimate of the dispatch's time without a
neighbour.  Output is markdown (profiles/adamw_tower_overlap.md).
"""
import argparse
import csv
import glob
import os
import re
import sys
from collections import defaultdict


def short(name):
    name = re.sub(r"\(anonymous namespace\)::|void |eavqa_attn_mfma::", "", name)
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if m:
        name = name[len(m.group(0)):][:int(m.group(1))]
    return name.split("(")[0][:48]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    files = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {args.dir}")
    rows = []
    with open(files[0], newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], short(r["Kernel_Name"]),
                         int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0), r.get("VGPR_Count", "?"), r.get("Workgroup_Size_X") or r.get("Workgroup_Size", "?")))
    rows.sort()
    alone = defaultdict(lambda: 1 << 62)
    for s, e, q, name, grid, _, _ in rows:
        alone[(name, grid)] = min(alone[(name, grid)], e - s)
    adam = [r for r in rows if r[3].startswith("adamw")]
    if len(adam) < args.steps + 2:
        sys.exit(f"only {len(adam)} AdamW dispatches in the trace")
    a0 = adam[0]
    print(f"`{a0[3]}`: grid {a0[4]} work-items in workgroups of {a0[6]}, {a0[5]} VGPRs; {len(adam)} launches, "
          f"durations min / median / max {min(e - s for s, e, *_ in adam) / 1e3:.1f} / "
          f"{sorted(e - s for s, e, *_ in adam)[len(adam) // 2] / 1e3:.1f} / {max(e - s for s, e, *_ in adam) / 1e3:.1f} us\n")
    for k, (s, e, q, *_) in enumerate(adam[-1 - args.steps:-1]):
        other = [r for r in rows if r[2] != q and r[1] > s and r[0] < e]
        inside = [r for r in other if r[0] >= s and r[1] <= e]
        starts = [r for r in other if r[0] >= s]
        ends = [r for r in other if r[1] <= e]
        # the next dispatch of the other queue(s) that starts after AdamW ended: how long the side stream waited
        later = [r for r in rows if r[2] != q and r[0] >= e]
        print(f"### step {k + 1}: AdamW {(e - s) / 1e3:.1f} us")
        print(f"- side-stream dispatches overlapping the interval: {len(other)}; starting inside: {len(starts)}; ending inside: {len(ends)}; "
              f"both: {len(inside)}")
        print(f"- tower work retired inside (dispatches ending inside): {sum(r[1] - r[0] for r in ends) / 1e3:.1f} us in situ, "
              f"{sum(alone[(r[3], r[4])] for r in ends) / 1e3:.1f} us of alone-time")
        if later:
            print(f"- first side-stream dispatch starting after the interval: `{later[0][3]}` at +{(later[0][0] - e) / 1e3:.1f} us")
        if other:
            print("\n| kernel | grid | start after AdamW's start (us) | duration (us) | alone (us) | ends inside |")
            print("|---|---|---|---|---|---|")
            for r in other[:40]:
                print(f"| `{r[3]}` | {r[4]} | {(r[0] - s) / 1e3:.1f} | {(r[1] - r[0]) / 1e3:.1f} | {alone[(r[3], r[4])] / 1e3:.1f} | {'yes' if r[1] <= e else 'no'} |")
            if len(other) > 40:
                print(f"| ... {len(other) - 40} more | | | | | |")
        print()


if __name__ == "__main__":
    main()
