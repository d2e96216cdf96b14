#!/usr/bin/env python3
"""Logits processors on the T0_3B shape (T5 v1.1 XL, random-init weights, bf16): the setting of tools/sample_bench.py and
tools/beam_bench.py - 32 questions, 150 encoder positions, max_length 10.

Prints ms per decoder step (decoder step + lm head + [eavqa_logits_process] + pick [+ beam reorder], device events around the whole
step) for greedy at 32 rows, sampling at 32 rows and beam search with 4 beams (128 decoder rows), each with the processors OFF (the loop
of the tree without them: no extra launch) and ON (``PROCESSORS`` below); per generation the mean over its 9 steps, then median and
min .. max over REPS generations after a warm-up one.  The six kinds of generation alternate, so that drift of the box hits all alike.
Also the processor call alone (events around it).  The last line is one JSON object.

``--off-only`` measures the three OFF loops only; together with ``--tree PATH`` (import the package from another checkout, e.g. a
worktree of the parent commit, which has no eavqa_logits_process) it gives the parent's step times for the comparison
"processors off = the parent's step", to be run interleaved with this tree's in one GPU call."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch

from eavqa_amd import ops
from eavqa_amd.data.synthetic import fewshot_batch
from eavqa_amd.models.t5 import _StepDriver
from eavqa_amd.models.vct0 import VCT0Prefix

if not torch.cuda.is_available():
    sys.exit("logits_process_bench.py measures on the GPU; there is none here")

dev, dtype = "cuda:0", torch.bfloat16
B, K, shots, seg, L, D, max_length, REPS = 32, 4, 4, 20, 10, 768, 10, args.reps
SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9)
PROCESSORS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=5, bad_words_ids=[[17], [23, 29]])
torch.manual_seed(2021)
model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version="bigscience/T0_3B", dtype=dtype, device=dev).eval()
lm, c = model.lm, model.lm.cfg
b = fewshot_batch(B, c.vocab, shots, seg, 32099, image_size=8, device=dev)
emb = torch.randn(B, shots + 1, D, device=dev, dtype=dtype)
proc = None
if not args.off_only:
    from eavqa_amd.models.logits_process import processing_plan
    proc = processing_plan(dict(PROCESSORS, eos_token_id=c.eos_token_id, max_length=max_length)).upload(c.vocab, dev)


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


with torch.no_grad():
    rows = model._project(emb)
    enc, mask, S = model._encode_interleaved(b["input_ids"], b["attention_mask"], rows, shots + 1, 32099)
    kv = lm.cross_kv(enc)
I, nl, t_max = c.inner, len(lm.dec), max_length
rel = lm.rel_table(True, t_max)


def make_rows():
    cache = [(torch.empty((B * t_max, I), device=dev, dtype=dtype), torch.empty((B * t_max, I), device=dev, dtype=dtype)) for _ in lm.dec]
    return dict(driver=_StepDriver(lm, cache, kv, B, t_max), seq=torch.zeros((B, max_length), dtype=torch.int64, device=dev),
                raw=torch.empty(B, dtype=torch.int32, device=dev))


def make_beams():
    planes = [torch.empty((2 * nl, B * K, t_max, I), device=dev, dtype=dtype) for _ in range(2)]
    caches = [[(p[2 * i].view(B * K * t_max, I), p[2 * i + 1].view(B * K * t_max, I)) for i in range(nl)] for p in planes]
    return dict(planes=planes, drivers=[_StepDriver(lm, ch, kv, B, t_max, beams=K) for ch in caches])


def rows_generation(st, sample, on, seed=0):
    """(ms per step, ms of the processor call per step)"""
    unf = torch.ones(B, dtype=torch.int32, device=dev)
    st["seq"].zero_()
    marks = []
    for t in range(1, max_length):
        a = ev()
        lg = lm.logits(st["driver"].step(lm.embed(st["seq"][:, t - 1].contiguous()), mask, t, S, rel))
        p0 = ev()
        if on:
            proc.apply(lg, c.vocab, st["seq"], t, 1)
        p1 = ev()
        if sample:
            ops.sample_pick(lg, c.vocab, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"], seed, t, c.pad_token_id, c.eos_token_id,
                            st["raw"], st["seq"][:, t], unf)
        else:
            ops.greedy_pick(lg, c.vocab, c.pad_token_id, c.eos_token_id, st["raw"], st["seq"][:, t], unf)
        marks.append((a, p0, p1, ev()))
    torch.cuda.synchronize()
    return sum(m[0].elapsed_time(m[3]) for m in marks) / len(marks), sum(m[1].elapsed_time(m[2]) for m in marks) / len(marks)


def beam_generation(st, on):
    bs = ops.BeamState(B, K, max_length, c.decoder_start_token_id, c.pad_token_id or c.eos_token_id, dev)
    cur, marks = 0, []
    for t in range(1, max_length):
        a = ev()
        lg = lm.logits(st["drivers"][cur].step(lm.embed(bs.next_tokens), mask, t, S, rel))
        p0 = ev()
        if on:
            proc.apply(lg, c.vocab, bs.run_seq, t, 1, to_logprobs=True)
        p1 = ev()
        if on:
            ops.beam_step(lg, c.vocab, bs, t, c.eos_token_id, logprobs=True)
        else:
            ops.beam_step(lg, c.vocab, bs, t, c.eos_token_id)
        ops.beam_reorder(st["planes"][cur], st["planes"][1 - cur], bs.parents, t)
        cur = 1 - cur
        marks.append((a, p0, p1, ev()))
    torch.cuda.synchronize()
    return sum(m[0].elapsed_time(m[3]) for m in marks) / len(marks), sum(m[1].elapsed_time(m[2]) for m in marks) / len(marks)


rows_st, beams_st = make_rows(), make_beams()
kinds = {}
for on in ((False,) if args.off_only else (False, True)):
    tag = "on" if on else "off"
    kinds[f"greedy_32_{tag}"] = lambda seed, on=on: rows_generation(rows_st, False, on, seed)
    kinds[f"sample_32_{tag}"] = lambda seed, on=on: rows_generation(rows_st, True, on, seed)
    kinds[f"beams_{B * K}_{tag}"] = lambda seed, on=on: beam_generation(beams_st, on)
stat = lambda xs: dict(median=float(torch.tensor(xs).median()), min=min(xs), max=max(xs))
fmt = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, max {d['max']:.3f})"
with torch.no_grad():
    for fn in kinds.values():
        fn(0)                                                              # warm every shape up
    runs = {k: [] for k in kinds}
    for rep in range(REPS):
        for k, fn in kinds.items():
            runs[k].append(fn(rep))
print(f"per decoder step, median over {REPS} generations of {max_length - 1} steps; {B} encoder outputs of {S} positions; tree {args.tree}")
out = {}
for k, rs in runs.items():
    out[k] = dict(step=stat([r[0] for r in rs]), processors=stat([r[1] for r in rs]))
    print(f"  {k:14s} step {fmt(out[k]['step'])}" + (f"; eavqa_logits_process {fmt(out[k]['processors'])}" if k.endswith("_on") else ""))
if not args.off_only:
    for base in ("greedy_32", "sample_32", f"beams_{B * K}"):
        d = stat([a[0] - o[0] for a, o in zip(runs[base + "_on"], runs[base + "_off"])])
        out[base + "_on_minus_off"] = d
        print(f"  {base}: on - off, paired by generation: {fmt(d)}")
print(json.dumps(dict(B=B, beams=K, S=S, max_length=max_length, reps=REPS, tree=args.tree, off_only=args.off_only,
                      processors=None if args.off_only else PROCESSORS, step_ms=out)))
