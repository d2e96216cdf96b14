#!/usr/bin/env python3
"""Sampling on the T0_3B shape (T5 v1.1 XL, random-init weights, bf16): 32 questions, the encoder input of the few-shot benchmark leg
(4 shots + query, 20 text tokens per segment, prefix 10: 150 encoder positions), max_length 10 - the setting of tools/beam_bench.py.

Prints (a) ms per decoder step, split into decoder step / lm head / pick, for greedy at 32 rows, sampling with one draw per question
(32 rows) and sampling with 4 draws per question (128 decoder rows over the 32 encoder outputs, the row count of the beam bench):
device events around each call, per generation the mean over its 9 steps, then median and min .. max over REPS generations after a
warm-up one; the three kinds of generation alternate, so that drift of the box hits all alike; (b) the two pick kernels alone,
eavqa_greedy_pick against eavqa_sample_pick, at B = 32 and 128, V = 32 128 and 50 272, with top-k / top-p off, top_k = 50 and
top_p = 0.9 (median of ITERS launches between two events, logits resident), beside the byte model B * V * 4.  The last line is one
JSON object."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from eavqa_amd import ops
from eavqa_amd.data.synthetic import fewshot_batch
from eavqa_amd.models.t5 import _StepDriver
from eavqa_amd.models.vct0 import VCT0Prefix

if not torch.cuda.is_available():
    sys.exit("sample_bench.py measures on the GPU; there is none here")

dev, dtype = "cuda:0", torch.bfloat16
B, N, shots, seg, L, D, max_length, REPS, ITERS = 32, 4, 4, 20, 10, 768, 10, 20, 50
HBM = 8.0e12
SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9)
torch.manual_seed(2021)
model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version="bigscience/T0_3B", dtype=dtype, device=dev).eval()
lm, c = model.lm, model.lm.cfg
b = fewshot_batch(B, c.vocab, shots, seg, 32099, image_size=8, device=dev)
emb = torch.randn(B, shots + 1, D, device=dev, dtype=dtype)


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


with torch.no_grad():
    rows = model._project(emb)
    enc, mask, S = model._encode_interleaved(b["input_ids"], b["attention_mask"], rows, shots + 1, 32099)
    kv = lm.cross_kv(enc)
I, t_max = c.inner, max_length
rel = lm.rel_table(True, t_max)
names = ("decoder_step", "lm_head", "pick")


def make(n):
    """The buffers and the step driver of a generation with n decoder rows per question."""
    R = B * n
    cache = [(torch.empty((R * t_max, I), device=dev, dtype=dtype), torch.empty((R * t_max, I), device=dev, dtype=dtype)) for _ in lm.dec]
    return dict(R=R, driver=_StepDriver(lm, cache, kv, B, t_max, beams=n), seq=torch.zeros((R, max_length), dtype=torch.int64, device=dev),
                raw=torch.empty(R, dtype=torch.int32, device=dev))


def generation(st, sample, seed=0):
    unf = torch.ones(st["R"], dtype=torch.int32, device=dev)
    marks = []
    for t in range(1, max_length):
        y = lm.embed(st["seq"][:, t - 1].contiguous())
        m = [ev()]
        last = st["driver"].step(y, mask, t, S, rel)
        m.append(ev())
        lg = lm.logits(last)
        m.append(ev())
        if sample:
            ops.sample_pick(lg, c.vocab, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"], seed, t, c.pad_token_id, c.eos_token_id,
                            st["raw"], st["seq"][:, t], unf)
        else:
            ops.greedy_pick(lg, c.vocab, c.pad_token_id, c.eos_token_id, st["raw"], st["seq"][:, t], unf)
        m.append(ev())
        marks.append(m)
    torch.cuda.synchronize()
    return [sum(m[i].elapsed_time(m[i + 1]) for m in marks) / len(marks) for i in range(len(names))]


stat = lambda xs: dict(median=float(torch.tensor(xs).median()), min=min(xs), max=max(xs))
fmt = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, max {d['max']:.3f})"
kinds = {"greedy_32": (make(1), False), "sample_32": (make(1), True), f"sample_{B * N}": (make(N), True)}
with torch.no_grad():
    for st, sample in kinds.values():
        generation(st, sample)                                             # warm every shape up
    runs = {k: [] for k in kinds}
    for rep in range(REPS):
        for k, (st, sample) in kinds.items():
            runs[k].append(generation(st, sample, seed=rep))
steps = {}
print(f"per decoder step, median over {REPS} generations of {max_length - 1} steps; {B} encoder outputs of {S} positions; sampling {SAMPLING}")
for k, rs in runs.items():
    steps[k] = dict(total=stat([sum(r) for r in rs]), **{n: stat([r[i] for r in rs]) for i, n in enumerate(names)})
    print(f"  {k:11s} total {fmt(steps[k]['total'])}")
    for n in names:
        print(f"      {n:13s} {fmt(steps[k][n])}")
diff = stat([sum(s) - sum(g) for s, g in zip(runs["sample_32"], runs["greedy_32"])])
pick_diff = stat([s[2] - g[2] for s, g in zip(runs["sample_32"], runs["greedy_32"])])
print(f"  sampling - greedy at 32 rows, paired by generation: step {fmt(diff)}; pick alone {fmt(pick_diff)}")

# ---- (b) the pick kernels alone
kernels = []
settings = [("greedy", None), ("sample, filters off", (1.0, 0, 1.0)), ("sample, top_k=50", (1.0, 50, 1.0)), ("sample, top_p=0.9", (1.0, 0, 0.9))]
print(f"pick kernels alone, median of {ITERS} launches; byte model B * V * 4 at {HBM / 1e12:.0f} TB/s")
for rows_ in (32, 128):
    for V in (32128, 50272):
        lg = torch.randn(rows_, V, device=dev) * 3
        raw, em, unf = torch.empty(rows_, dtype=torch.int32, device=dev), torch.empty(rows_, dtype=torch.int64, device=dev), torch.ones(rows_, dtype=torch.int32, device=dev)
        for name, s in settings:
            def launch(i):
                if s is None:
                    ops.greedy_pick(lg, V, 0, 1, raw, em, unf)
                else:
                    ops.sample_pick(lg, V, s[0], s[1], s[2], 1, i, 0, 1, raw, em, unf)
            for i in range(5):
                launch(i)
            ts = []
            for i in range(ITERS):
                unf.fill_(1)
                a = ev()
                launch(i)
                z = ev()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(z) * 1e3)
            us = float(torch.tensor(ts).median())
            floor = rows_ * V * 4 / HBM * 1e6
            kernels.append(dict(rows=rows_, V=V, kernel=name, us=us, min_us=min(ts), byte_floor_us=floor))
            print(f"  B={rows_:3d} V={V:5d} {name:20s} {us:8.1f} us (min {min(ts):.1f}); {rows_ * V * 4 / 1e6:.1f} MB -> floor {floor:.2f} us")
print(json.dumps(dict(B=B, draws=N, S=S, max_length=max_length, reps=REPS, sampling=SAMPLING, step_ms=steps, sample_minus_greedy_ms=diff,
                      pick_minus_greedy_ms=pick_diff, kernels=kernels)))
