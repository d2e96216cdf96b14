#!/usr/bin/env python3
"""Ensemble decoding on the T0_3B shape (T5 v1.1 XL, random-init weights, bf16): 32 questions x 4 permutations of the in-context
examples, the encoder input of the few-shot benchmark leg (4 shots + query, 20 text tokens per segment, prefix 10: 150 encoder
positions), max_length 10.

Compares, as wall time of one whole answer batch (host work and the final synchronisation included), medians of REPS generations after
a warm-up one, ONE generation of each kind in turn so that drift of the box hits all alike:
  (a) ``FewShotVQAExecutor.generate_from_ensembles`` - n greedy generations one after the other, the [steps, B, V] scores copied to
      the host and log-softmaxed there;
  (b) ``generate_ensemble(ensemble="select")`` - the same rule, the B * n rows in one loop;
  (c) ``generate_ensemble(ensemble="product")`` and (d) ``"mixture"`` - one sequence per question under all members.
Then ``eavqa_ensemble_combine`` itself: per decoder step inside (c) / (d) (device events around every launch of one generation), and
alone, 200 launches back to back on [128, 32128] member logits (16.4 MB read twice + 4.1 MB written), next to
``eavqa_logits_process(to_logprobs=1)`` and ``eavqa_trie_constrain`` on a buffer of the same size.  The last line is one JSON object."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from eavqa_amd import ops
from eavqa_amd.data.synthetic import fewshot_batch
from eavqa_amd.models.constrained import AnswerTrie
from eavqa_amd.models.vct0 import VCT0Prefix
from eavqa_amd.trainers.vct0_executor import FewShotVQAExecutor
from eavqa_amd.utils.attrdict import AttrDict

if not torch.cuda.is_available():
    sys.exit("ensemble_bench.py measures on the GPU; there is none here")

dev, dtype = "cuda:0", torch.bfloat16
B, N, shots, seg, L, D, max_length, REPS = 32, 4, 4, 20, 10, 768, 10, 20
torch.manual_seed(2021)
model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version="bigscience/T0_3B", dtype=dtype, device=dev).eval()
lm, c = model.lm, model.lm.cfg
V, vpad = c.vocab, model.lm.vpad
fx = FewShotVQAExecutor(AttrDict(), model=model, dtype=dtype, device=dev)

# member i of a question: the same five images, the shots in another order, and its own text
g = torch.Generator().manual_seed(3)
batches = [fewshot_batch(B, V, shots, seg, 32099, image_size=8, seed=11 + i, device=dev) for i in range(N)]
ids = torch.stack([b["input_ids"] for b in batches], dim=1)                          # [B, N, T]
mask = torch.stack([b["attention_mask"] for b in batches], dim=1)
images = torch.randn(B, shots + 1, D, generator=g).to(device=dev, dtype=dtype)
emb = torch.stack([images[:, torch.randperm(shots, generator=g).tolist() + [shots]] for _ in range(N)], dim=1)      # [B, N, 5, D]
S = ids.shape[-1] + (L - 1) * (shots + 1)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


kinds = dict(
    from_ensembles=lambda: fx.generate_from_ensembles(ids, mask, emb, N, max_length),
    select=lambda: model.generate_ensemble(prefix=emb, question_tokens=ids, question_mask=mask, ensemble="select", max_length=max_length),
    product=lambda: model.generate_ensemble(prefix=emb, question_tokens=ids, question_mask=mask, ensemble="product", max_length=max_length),
    mixture=lambda: model.generate_ensemble(prefix=emb, question_tokens=ids, question_mask=mask, ensemble="mixture", max_length=max_length),
)
stat = lambda xs: dict(median=float(torch.tensor(xs).median()), min=min(xs), max=max(xs))
fmt = lambda d, unit="ms": f"{d['median']:.2f} {unit} (min {d['min']:.2f}, max {d['max']:.2f})"
out = dict(B=B, members=N, S=S, max_length=max_length, reps=REPS, V=V)
with torch.no_grad():
    lengths = {}
    for name, fn in kinds.items():                                                   # warm every shape up
        res = fn()
        lengths[name] = max(len(r) for r in res)
    runs = {name: [] for name in kinds}
    for rep in range(REPS):
        for name, fn in kinds.items():
            runs[name].append(wall(fn)[0])
out["sequence_length"] = lengths
print(f"one answer batch: {B} questions x {N} members, {S} encoder positions, max_length {max_length}; median over {REPS} generations")
for name in kinds:
    out[name + "_ms"] = stat(runs[name])
    print(f"  {name:15s} {fmt(out[name + '_ms'])}   (longest sequence {lengths[name]})")
for name in ("select", "product", "mixture"):
    d = stat([a - b for a, b in zip(runs[name], runs["from_ensembles"])])             # paired: generation i of each
    out[name + "_minus_from_ensembles_ms"] = d
    print(f"  {name} - from_ensembles, paired by generation: {fmt(d)} = {100 * d['median'] / out['from_ensembles_ms']['median']:+.1f} %")

# ---- the combine kernel inside a generation: device events around every launch
real = ops.ensemble_combine
for mode in ("product", "mixture"):
    marks = []

    def timed(*a, **k):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **k)
        e1.record()
        marks.append((e0, e1))
        return r
    ops.ensemble_combine = timed
    try:
        with torch.no_grad():
            kinds[mode]()
        torch.cuda.synchronize()
    finally:
        ops.ensemble_combine = real
    us = [a.elapsed_time(b) * 1e3 for a, b in marks]
    out[f"combine_in_loop_{mode}_us"] = dict(stat(us), steps=len(us))
    print(f"eavqa_ensemble_combine inside a {mode} generation, {len(us)} steps: {fmt(out[f'combine_in_loop_{mode}_us'], 'us')} per step")

# ---- the kernel alone
REPEAT = 200
R = B * N
lg0 = (4.0 * torch.randn(R, vpad, device=dev)).contiguous()
res = torch.empty((B, vpad), device=dev, dtype=torch.float32)
stats = torch.empty(2 * R, device=dev, dtype=torch.float32)
buf = lg0.clone()
hist = torch.zeros((R, max_length), dtype=torch.int64, device=dev)
first = (torch.randperm(V - 200, generator=torch.Generator().manual_seed(7))[:1500] + 2).tolist()
con = AnswerTrie(sequences=[[t] for t in first], eos_token_id=c.eos_token_id).upload(V, dev)


def alone(fn):
    fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    z = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPEAT):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / REPEAT * 1e3                                          # microseconds per call


kernel = dict(
    combine_product_us=alone(lambda: ops.ensemble_combine(lg0, V, N, "product", out=res, stats=stats)),
    combine_mixture_us=alone(lambda: ops.ensemble_combine(lg0, V, N, "mixture", out=res, stats=stats)),
    combine_product_one_member_us=alone(lambda: ops.ensemble_combine(lg0[:B], V, 1, "product", out=res, stats=stats)),
    logits_process_logprobs_us=alone(lambda: ops.logits_process(buf, V, hist, 1, to_logprobs=True)),
    trie_constrain_root_us=alone(lambda: con.apply(buf, V, hist, 1, 1)),
)
read_b, write_b = R * V * 4, B * V * 4
out["kernel"] = dict(kernel, member_rows=R, read_bytes_once=read_b, written_bytes=write_b, model_bytes=2 * read_b + write_b)
print(f"alone, {R} member rows x {V} columns ({read_b / 1e6:.1f} MB, read twice) -> {B} rows ({write_b / 1e6:.1f} MB), microseconds per call "
      f"(two launches) back to back over {REPEAT}:")
for n, v in kernel.items():
    print(f"    {n:32s} {v:8.1f}")
for mode in ("product", "mixture"):
    us = kernel[f"combine_{mode}_us"]
    print(f"    {mode}: {(2 * read_b + write_b) / us / 1e3:.0f} GB/s of the byte model (2 x {read_b / 1e6:.1f} MB + {write_b / 1e6:.1f} MB)")
print(json.dumps(out))
