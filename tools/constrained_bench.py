#!/usr/bin/env python3
"""Decoding inside an answer set on the T0_3B shape (T5 v1.1 XL, random-init weights, bf16): 32 questions, the encoder input of the
few-shot benchmark leg (4 shots + query, 20 text tokens per segment, prefix 10: 150 encoder positions), max_length 10, a synthetic set of
3 000 answers of 1-4 tokens whose root has about 1 500 children (VQA2's answer vocabulary in size and shape).

Prints ms per decoder step split into decoder step / lm head / eavqa_trie_constrain / pick (/ eavqa_beam_reorder), device events around
each call, for (a) greedy search at 32 rows and (b) 4 beams at 128 rows, each WITH and WITHOUT the constraint: one generation of each of
the four in turn, so that drift of the box hits all alike; per generation the mean over its 9 steps, then median and min .. max over REPS
generations after a warm-up one, and the paired difference constrained - unconstrained.  Every generation runs all 9 steps (the product
loops stop once every row has ended, which a constrained run does early - that would compare different step counts).  (c) the kernel
alone, 200 back-to-back launches on a mid-generation state: plain mask, mask with the log-softmax pass, and eavqa_logits_process's
log-softmax pass for comparison.  ``--score``: also ``score_candidates`` over the same 3 000 answers for the same batch (three calls of
1 000: it ranks at most 1 024 per call), for orientation.  The last line is one JSON object."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from eavqa_amd import ops
from eavqa_amd.data.synthetic import fewshot_batch
from eavqa_amd.models.constrained import AnswerTrie
from eavqa_amd.models.t5 import _StepDriver
from eavqa_amd.models.vct0 import VCT0Prefix

if not torch.cuda.is_available():
    sys.exit("constrained_bench.py measures on the GPU; there is none here")

dev, dtype = "cuda:0", torch.bfloat16
B, K, shots, seg, L, D, max_length, REPS = 32, 4, 4, 20, 10, 768, 10, 20
N_ANSWERS, N_FIRST = 3000, 1500
torch.manual_seed(2021)
model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version="bigscience/T0_3B", dtype=dtype, device=dev).eval()
lm, c = model.lm, model.lm.cfg
V, eos = c.vocab, c.eos_token_id
b = fewshot_batch(B, V, shots, seg, 32099, image_size=8, device=dev)
emb = torch.randn(B, shots + 1, D, device=dev, dtype=dtype)

# the answer set: N_FIRST one-token answers, and as many longer ones (2-4 tokens) that start with one of those tokens
g = torch.Generator().manual_seed(7)
first = (torch.randperm(V - 200, generator=g)[:N_FIRST] + 2).tolist()
answers = [[t] for t in first]
for i in range(N_ANSWERS - N_FIRST):
    n = 1 + i % 3
    answers.append([first[int(torch.randint(0, N_FIRST, (1,), generator=g))]] + (torch.randint(2, V - 200, (n,), generator=g)).tolist())
trie = AnswerTrie(sequences=answers, eos_token_id=eos)
con = trie.upload(V, dev)
root_fan_out = int(trie.child_begin[1] - trie.child_begin[0])
print(f"answer set: {len(trie.sets[0])} members, {trie.is_end.numel()} trie nodes, root fan-out {root_fan_out}")


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


with torch.no_grad():
    rows = model._project(emb)
    enc, mask, S = model._encode_interleaved(b["input_ids"], b["attention_mask"], rows, shots + 1, 32099)
    kv = lm.cross_kv(enc)
R, I, nl, t_max = B * K, c.inner, len(lm.dec), max_length
planes = [torch.empty((2 * nl, R, t_max, I), device=dev, dtype=dtype) for _ in range(2)]
caches = [[(p[2 * i].view(R * t_max, I), p[2 * i + 1].view(R * t_max, I)) for i in range(nl)] for p in planes]
drivers = [_StepDriver(lm, ch, kv, B, t_max, beams=K) for ch in caches]
cache_g = [(torch.empty((B * t_max, I), device=dev, dtype=dtype), torch.empty((B * t_max, I), device=dev, dtype=dtype)) for _ in lm.dec]
drv = _StepDriver(lm, cache_g, kv, B, t_max)
rel = lm.rel_table(True, t_max)
raw = torch.empty(B, dtype=torch.int32, device=dev)
gnames = ("decoder_step", "lm_head", "constrain", "greedy_pick")
bnames = ("decoder_step", "lm_head", "constrain", "beam_step", "beam_reorder")
state = {}


def greedy_generation(constrained):
    seq = torch.full((B, max_length), c.pad_token_id, dtype=torch.int64, device=dev)
    seq[:, 0] = c.decoder_start_token_id
    unf = torch.ones(B, dtype=torch.int32, device=dev)
    marks = []
    for t in range(1, max_length):
        y = lm.embed(seq[:, t - 1].contiguous())
        m = [ev()]
        last = drv.step(y, mask, t, S, rel)
        m.append(ev())
        lg = lm.logits(last)
        m.append(ev())
        if constrained:
            con.apply(lg, V, seq, t, 1)
        m.append(ev())
        ops.greedy_pick(lg, V, c.pad_token_id, eos, raw, seq[:, t], unf)
        m.append(ev())
        marks.append(m)
    torch.cuda.synchronize()
    return [sum(m[i].elapsed_time(m[i + 1]) for m in marks) / len(marks) for i in range(len(gnames))]


def beam_generation(constrained):
    st = ops.BeamState(B, K, max_length, c.decoder_start_token_id, c.pad_token_id or eos, dev)
    cur, marks = 0, []
    for t in range(1, max_length):
        y = lm.embed(st.next_tokens)
        m = [ev()]
        last = drivers[cur].step(y, mask, t, S, rel)
        m.append(ev())
        lg = lm.logits(last)
        if constrained and t == 2:                           # (outside the timed intervals' sum only in the one generation that keeps it)
            state.setdefault("beam_hist", st.run_seq.clone())
            state.setdefault("beam_logits", lg.clone())
        m.append(ev())
        if constrained:
            con.apply(lg, V, st.run_seq, t, 1, to_logprobs=True)
        m.append(ev())
        ops.beam_step(lg, V, st, t, eos, logprobs=constrained)
        m.append(ev())
        ops.beam_reorder(planes[cur], planes[1 - cur], st.parents, t)      # (the product loop skips it after the last step)
        m.append(ev())
        cur = 1 - cur
        marks.append(m)
    torch.cuda.synchronize()
    return [sum(m[i].elapsed_time(m[i + 1]) for m in marks) / len(marks) for i in range(len(bnames))]


kinds = (("greedy", greedy_generation, False), ("greedy_constrained", greedy_generation, True), ("beams", beam_generation, False),
         ("beams_constrained", beam_generation, True))
with torch.no_grad():
    for _, fn, flag in kinds:                                # warm every shape up
        fn(flag)
    runs = {name: [] for name, _, _ in kinds}
    for rep in range(REPS):
        for name, fn, flag in kinds:
            runs[name].append(fn(flag))
stat = lambda xs: dict(median=float(torch.tensor(xs).median()), min=min(xs), max=max(xs))
fmt = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, max {d['max']:.3f})"
out = dict(B=B, beams=K, S=S, max_length=max_length, reps=REPS, answers=len(trie.sets[0]), trie_nodes=trie.is_end.numel(), root_fan_out=root_fan_out)
print(f"per decoder step, median over {REPS} generations of {max_length - 1} steps ({B} questions, {S} encoder positions)")
for name, _, _ in kinds:
    names = gnames if name.startswith("greedy") else bnames
    out[name] = dict(total=stat([sum(r) for r in runs[name]]), **{n: stat([r[i] for r in runs[name]]) for i, n in enumerate(names)})
    print(f"  {name:18s} step {fmt(out[name]['total'])}")
    for n in names:
        print(f"      {n:13s} {fmt(out[name][n])}")
for plain, cons in (("greedy", "greedy_constrained"), ("beams", "beams_constrained")):
    d = stat([sum(a) - sum(p) for a, p in zip(runs[cons], runs[plain])])          # paired: generation i of each
    out[cons + "_minus_" + plain] = d
    print(f"  {cons} - {plain}, paired by generation: {fmt(d)} = {100 * d['median'] / out[plain]['total']['median']:+.2f} % of the step")

# ---- (c) the kernel alone, on the beam state after two steps (rows at depth 1 of the trie) and on the root (empty history)
N = 200
hist, lg0 = state["beam_hist"], state["beam_logits"]


def alone(fn):
    fn()
    torch.cuda.synchronize()
    a = ev()
    for _ in range(N):
        fn()
    z = ev()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / N * 1e3                       # microseconds per launch


buf = lg0.clone()
kernel = dict(
    mask_root_us=alone(lambda: con.apply(buf, V, hist, 1, 1)),
    mask_depth1_us=alone(lambda: con.apply(buf, V, hist, 2, 1)),
    mask_logprobs_root_us=alone(lambda: (buf.copy_(lg0), con.apply(buf, V, hist, 1, 1, to_logprobs=True))),
    mask_logprobs_depth1_us=alone(lambda: (buf.copy_(lg0), con.apply(buf, V, hist, 2, 1, to_logprobs=True))),
    logits_process_logprobs_us=alone(lambda: (buf.copy_(lg0), ops.logits_process(buf, V, hist, 2, to_logprobs=True))),
    copy_us=alone(lambda: buf.copy_(lg0)),
)
out["kernel"] = dict(kernel, rows=R, written_bytes=R * V * 4)
print(f"eavqa_trie_constrain alone, {R} rows x {V} columns ({R * V * 4 / 1e6:.1f} MB), microseconds per launch back to back over {N}:")
for n, v in kernel.items():
    print(f"    {n:28s} {v:8.1f}")
print("    (the three *_logprobs rows include the copy that restores the logits; subtract copy_us)")

if "--score" in sys.argv:
    n_ans = len(trie.sets[0])
    cand = torch.full((n_ans, 5), -100, dtype=torch.int64)
    for i, a in enumerate(trie.sets[0]):
        cand[i, :len(a)] = torch.tensor(a)
        cand[i, len(a)] = eos
    kw = dict(prefix=emb, question_tokens=b["input_ids"], question_mask=b["attention_mask"], num_shots=shots, length_penalty=1.0)

    def score_all():
        return [model.score_candidates(candidates=cand[i:i + 1000], **kw) for i in range(0, n_ans, 1000)]
    score_all()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score_all()
    torch.cuda.synchronize()
    out["score_candidates_3000_ms"] = (time.perf_counter() - t0) * 1e3
    print(f"score_candidates, {B} questions x {n_ans} candidates (calls of 1 000, encoder included): {out['score_candidates_3000_ms']:.0f} ms")
print(json.dumps(out))
