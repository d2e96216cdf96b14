#!/usr/bin/env python3
"""Beam search on the T0_3B shape (T5 v1.1 XL, random-init weights, bf16): 32 questions x 4 beams, the encoder input of the few-shot
benchmark leg (4 shots + query, 20 text tokens per segment, prefix 10: 150 encoder positions), max_length 10.

Prints (a) the time of one beam generation per batch, (b) ms per decoder step split into decoder step / lm head / eavqa_beam_step /
eavqa_beam_reorder (device events around each call; per generation the mean over its 9 steps, then median and min .. max over REPS
generations after a warm-up one), each kernel's bytes and share of 8 TB/s, and (c) greedy generation of the SAME tree at 128 rows - the
same decoder row count on the same eavqa_gemm route (more than 64 rows have no split-K route).  Beam and greedy generations alternate,
so that drift of the box hits both alike.  The last line is one JSON object."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from eavqa_amd import ops
from eavqa_amd.data.synthetic import fewshot_batch
from eavqa_amd.models.t5 import _StepDriver
from eavqa_amd.models.vct0 import VCT0Prefix

if not torch.cuda.is_available():
    sys.exit("beam_bench.py measures on the GPU; there is none here")

dev, dtype = "cuda:0", torch.bfloat16
B, K, shots, seg, L, D, max_length, REPS = 32, 4, 4, 20, 10, 768, 10, 20
HBM = 8.0e12
torch.manual_seed(2021)
model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version="bigscience/T0_3B", dtype=dtype, device=dev).eval()
lm, c = model.lm, model.lm.cfg
b = fewshot_batch(B, c.vocab, shots, seg, 32099, image_size=8, device=dev)
emb = torch.randn(B, shots + 1, D, device=dev, dtype=dtype)
gen_kw = dict(prefix=emb, question_tokens=b["input_ids"], question_mask=b["attention_mask"], num_shots=shots, max_length=max_length)


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def wall(fn, n=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


# ---- (a) whole generations
beam_ms = wall(lambda: model.generate(num_beams=K, **gen_kw))
greedy32_ms = wall(lambda: model.generate(**gen_kw))
out = model.generate(num_beams=K, num_return_sequences=K, **gen_kw)
print(f"generate, {B} questions: {K} beams {beam_ms:.1f} ms per batch, greedy {greedy32_ms:.1f} ms per batch; beam output {tuple(out.shape)}")

# ---- (b) the beam step, piece by piece (the loop of FrozenT5.beam_search with events between the calls), and (c) greedy at the same
#      decoder row count: 128 rows, each with its own encoder output; one generation of each in turn
with torch.no_grad():
    rows = model._project(emb)
    enc, mask, S = model._encode_interleaved(b["input_ids"], b["attention_mask"], rows, shots + 1, 32099)
    kv = lm.cross_kv(enc)
R, I, nl, t_max = B * K, c.inner, len(lm.dec), max_length
planes = [torch.empty((2 * nl, R, t_max, I), device=dev, dtype=dtype) for _ in range(2)]
caches = [[(p[2 * i].view(R * t_max, I), p[2 * i + 1].view(R * t_max, I)) for i in range(nl)] for p in planes]
drivers = [_StepDriver(lm, ch, kv, B, t_max, beams=K) for ch in caches]
rel = lm.rel_table(True, t_max)
G = R
with torch.no_grad():
    enc_g = enc.view(B, S, -1).repeat(K, 1, 1).reshape(G * S, -1).contiguous()
    mask_g = mask.repeat(K, 1).contiguous()
    greedy128_ms = wall(lambda: lm.greedy(enc_g, mask_g, G, S, max_length))
    kv_g = lm.cross_kv(enc_g)
cache_g = [(torch.empty((G * t_max, I), device=dev, dtype=dtype), torch.empty((G * t_max, I), device=dev, dtype=dtype)) for _ in lm.dec]
drv = _StepDriver(lm, cache_g, kv_g, G, t_max)
seq = torch.zeros((G, max_length), dtype=torch.int64, device=dev)
raw = torch.empty(G, dtype=torch.int32, device=dev)
names = ("decoder_step", "lm_head", "beam_step", "beam_reorder")
gnames = ("decoder_step", "lm_head", "greedy_pick")


def beam_generation():
    st = ops.BeamState(B, K, max_length, c.decoder_start_token_id, c.pad_token_id or c.eos_token_id, dev)
    cur, marks = 0, []
    for t in range(1, max_length):
        y = lm.embed(st.next_tokens)
        m = [ev()]
        last = drivers[cur].step(y, mask, t, S, rel)
        m.append(ev())
        lg = lm.logits(last)
        m.append(ev())
        ops.beam_step(lg, c.vocab, st, t, c.eos_token_id)
        m.append(ev())
        ops.beam_reorder(planes[cur], planes[1 - cur], st.parents, t)      # (the product loop skips it after the last step)
        m.append(ev())
        cur = 1 - cur
        marks.append(m)
    torch.cuda.synchronize()
    return [sum(m[i].elapsed_time(m[i + 1]) for m in marks) / len(marks) for i in range(len(names))]


def greedy_generation():
    unf = torch.ones(G, dtype=torch.int32, device=dev)
    marks = []
    for t in range(1, max_length):
        y = lm.embed(seq[:, t - 1].contiguous())
        m = [ev()]
        last = drv.step(y, mask_g, t, S, rel)
        m.append(ev())
        lg = lm.logits(last)
        m.append(ev())
        ops.greedy_pick(lg, c.vocab, c.pad_token_id, c.eos_token_id, raw, seq[:, t], unf)
        m.append(ev())
        marks.append(m)
    torch.cuda.synchronize()
    return [sum(m[i].elapsed_time(m[i + 1]) for m in marks) / len(marks) for i in range(len(gnames))]


with torch.no_grad():
    beam_generation(), greedy_generation()                  # warm every shape up
    runs, gruns = [], []
    for rep in range(REPS):
        runs.append(beam_generation())
        gruns.append(greedy_generation())
stat = lambda xs: dict(median=float(torch.tensor(xs).median()), min=min(xs), max=max(xs))
per = {n: stat([r[i] for r in runs]) for i, n in enumerate(names)}
gper = {n: stat([r[i] for r in gruns]) for i, n in enumerate(gnames)}
tot, gtot = stat([sum(r) for r in runs]), stat([sum(r) for r in gruns])
diff = stat([sum(a) - sum(g) for a, g in zip(runs, gruns)])                      # paired: generation i of each
fmt = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, max {d['max']:.3f})"
step_bytes = R * c.vocab * 4
reorder_bytes = sum(2 * (2 * nl * R * t * I * 2) for t in range(1, max_length)) / (max_length - 1)         # read + write, mean over t
reorder_last = 2 * nl * R * max_length * I * 2
print(f"per decoder step, median over {REPS} generations of {max_length - 1} steps; beams: {R} decoder rows over {B} encoder outputs of {S} positions")
print(f"  beam step total {fmt(tot)}")
for n in names:
    print(f"    {n:13s} {fmt(per[n])}")
print(f"  greedy step at {G} rows, same tree: total {fmt(gtot)}")
for n in gnames:
    print(f"    {n:13s} {fmt(gper[n])}")
print(f"  difference beams - greedy, paired by generation: {fmt(diff)}; byte floor of the two beam kernels {(step_bytes + reorder_bytes) / HBM * 1e3:.3f} ms")
bs, br = per["beam_step"]["median"], per["beam_reorder"]["median"]
print(f"  eavqa_beam_step reads {step_bytes / 1e6:.1f} MB of logits: {step_bytes / bs / 1e9:.3f} TB/s = {step_bytes / (bs * 1e-3) / HBM:.3f} of 8 TB/s")
print(f"  eavqa_beam_reorder reads + writes {reorder_bytes / 1e9:.3f} GB (mean over t = 1..{max_length - 1}; {reorder_last / 1e9:.3f} GB each way at "
      f"t = {max_length}): {reorder_bytes / br / 1e9:.3f} TB/s = {reorder_bytes / (br * 1e-3) / HBM:.3f} of 8 TB/s; {br / tot['median']:.3f} of the step")
print(f"  whole greedy generation at {G} rows (lm.greedy): {greedy128_ms:.1f} ms")
print(json.dumps(dict(B=B, beams=K, S=S, max_length=max_length, reps=REPS, beam_generate_ms=beam_ms, greedy_generate_ms=greedy32_ms, beam_step_ms=per,
                      beam_step_total_ms=tot, beam_step_bytes=step_bytes, beam_reorder_bytes=reorder_bytes, greedy128_step_ms=gper,
                      greedy128_step_total_ms=gtot, beams_minus_greedy_ms=diff, greedy128_generate_ms=greedy128_ms)))
