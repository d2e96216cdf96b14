#!/usr/bin/env python3
"""What gradient-norm clipping costs beside the fused AdamW: `eavqa_adamw` alone against `eavqa_grad_sumsq` + `eavqa_clip_plan` +
`eavqa_adamw_clipped`, on flat buffers of the size of the cfg2 MLP mapper (85 M parameters), the cfg3 MLP mapper (218 M) and the cfg5
transformer mapper (1.17 B), bf16 shadow as in training (`profiles/grad_clipping.md`).

Byte model per parameter: AdamW 16 B read + 12 B written + 2 B shadow = 30 B; the sum of squares reads 4 B more; the plan kernel touches
<= 16 KiB.  So the clipped step should take (4 + 30) / 30 of the update's time if `grad_sumsq` streams at the rate the update reaches.

Every size runs in a child process of its own under a time limit; inside it the variants are timed with device events around single
launches, interleaved (A, B, the parts of B, A, B, ...), and the medians are reported.  One JSON line per size."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mlp_shapes(D, E, L):
    h = E * L // 2
    return [("model.0.weight", (h, D)), ("model.0.bias", (h,)), ("model.2.weight", (E * L, h)), ("model.2.bias", (E * L,))]


def transformer_shapes(D, E, clip_length, L, layers=8):
    out = [("linear.weight", (clip_length * E, D)), ("linear.bias", (clip_length * E,)), ("prefix_const", (L, E))]
    for i in range(layers):
        p = f"transformer.layers.{i}."
        out += [(p + "norm1.weight", (E,)), (p + "norm1.bias", (E,)), (p + "attn.to_queries.weight", (E, E)),
                (p + "attn.to_keys_values.weight", (2 * E, E)), (p + "attn.project.weight", (E, E)), (p + "attn.project.bias", (E,)),
                (p + "norm2.weight", (E,)), (p + "norm2.bias", (E,)), (p + "mlp.fc1.weight", (2 * E, E)), (p + "mlp.fc1.bias", (2 * E,)),
                (p + "mlp.fc2.weight", (E, 2 * E)), (p + "mlp.fc2.bias", (E,))]
    return out


# (ViT projection width, LM width, prefix length) of bench.py's workloads
SIZES = {"cfg2_mlp": lambda: mlp_shapes(512, 1280, 10), "cfg3_mlp": lambda: mlp_shapes(768, 2048, 10),
         "cfg5_transformer": lambda: transformer_shapes(768, 4096, 32, 32)}


def flat_numel(name):
    import torch
    from eavqa_amd.models.clipcap import FlatParams
    return FlatParams(SIZES[name](), "meta", torch.bfloat16).numel


def child(name, reps, warmup):
    import torch
    from eavqa_amd import ops
    from eavqa_amd.trainers.optim import bias_correction_table
    n = flat_numel(name)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    param = torch.randn(n, device=dev, generator=g)
    grad = torch.randn(n, device=dev, generator=g) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    shadow = torch.empty(n, device=dev, dtype=torch.bfloat16)
    partials = torch.zeros(ops.grad_sumsq_partials(n), device=dev, dtype=torch.float64)
    state = torch.zeros(ops.CLIP_STATE_WORDS, device=dev, dtype=torch.int32)
    table = bias_correction_table(0.9, 0.999).to(dev)
    kw = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    step = [0]

    def plain():
        step[0] += 1
        ops.adamw(param, grad, m, v, step[0], grad_scale=0.5, shadow=shadow, **kw)

    def sumsq():
        ops.grad_sumsq(grad, partials)

    def plan():
        ops.clip_plan(partials, 0.5, 1.0, table, state)

    def update():
        ops.adamw_clipped(param, grad, m, v, state, shadow=shadow, **kw)

    def clipped():
        sumsq(); plan(); update()

    variants = {"adamw": plain, "clipped_step": clipped, "grad_sumsq": sumsq, "clip_plan": plan, "adamw_clipped": update}
    times = {k: [] for k in variants}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for r in range(warmup + reps):
        for k, fn in variants.items():
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    torch.cuda.synchronize()
    med = {k: statistics.median(ts) for k, ts in times.items()}
    host = state.cpu()
    out = {"size": name, "numel": n, "partials": partials.numel(), "reps": reps,
           "us": {k: round(t, 1) for k, t in med.items()}, "us_min": {k: round(min(ts), 1) for k, ts in times.items()},
           "TBps": {"adamw": round(30.0 * n / med["adamw"] * 1e-6, 3), "adamw_clipped": round(30.0 * n / med["adamw_clipped"] * 1e-6, 3),
                    "grad_sumsq": round(4.0 * n / med["grad_sumsq"] * 1e-6, 3)},
           "clipped_over_adamw": round(med["clipped_step"] / med["adamw"], 4), "byte_model": round(34.0 / 30.0, 4),
           "norm": host.view(torch.float32)[0].item(), "applied_steps": int(host[4]), "skipped_steps": int(host[5])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds per size (child process)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.warmup)
    for name in args.sizes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {args.limit} s - stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode} - stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if args.out:
            with open(args.out, "a") as f:
                f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
