#!/usr/bin/env python3
"""Beam search on the causal few-shot leg (cfg4: OPT-2.7B, random-init weights, bf16): 32 questions x 4 beams behind the 4-shot prompt
(20 text tokens per segment, prefix 10), 10 new tokens.

Prints (a) the time of one ``generate_beams_fewshot`` and one greedy ``generate_fewshot`` per batch, and (b) ms per decode step (embedding,
all layers, final LayerNorm and lm head; device events around each step, per generation the mean over its steps, then median and
min .. max over REPS generations after a warm-up one) of three routes that alternate generation by generation, so that drift of the box
hits all alike:
  shared      ``eavqa_lm_block_step_shared``: 128 rows over the 32 prompts' caches (what ``beam_decode`` runs);
  replicated  ``eavqa_lm_block_forward`` on 128 rows whose prompt caches are copied 4-fold - the route a beam search had without the
              shared kernel; it exists in this tool only;
  greedy      the shipped greedy step at 32 rows (split-K route).
Next to them the byte model of the K / V traffic of a step.  The last line is one JSON object."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from eavqa_amd import ops
from eavqa_amd.data.synthetic import fewshot_batch
from eavqa_amd.models import decode
from eavqa_amd.models.clipcap import ClipCaptionPrefix
from eavqa_amd.models.lm import KNOWN_CONFIGS, FrozenCausalLM, LMConfig, random_init_state_dict

if not torch.cuda.is_available():
    sys.exit("causal_beam_bench.py measures on the GPU; there is none here")

dev, dtype = "cuda:0", torch.bfloat16
B, K, shots, seg, L, D, max_length = 32, 4, 4, 20, 10, 768, 10
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
torch.manual_seed(2021)
lcfg = LMConfig.from_hf_dict(KNOWN_CONFIGS["facebook/opt-2.7b"])
lm = FrozenCausalLM(lcfg, random_init_state_dict(lcfg, 2021, dev), dtype, dev)
model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=dev).eval()
sentinel = lcfg.vocab - 1
b = fewshot_batch(B, lcfg.vocab, shots, seg, sentinel, image_size=8, device=dev)
emb = torch.randn(B, shots + 1, D, device=dev, dtype=dtype)
kw = dict(num_shots=shots, special_token_id=sentinel, max_length=max_length, pad_token_id=1, eos_token_id=None)


def wall(fn, n=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


beam_ms = wall(lambda: model.generate_beams_fewshot(b["input_ids"], emb, b["attention_mask"], num_beams=K, **kw))
greedy_ms = wall(lambda: model.generate_fewshot(b["input_ids"], emb, b["attention_mask"], **kw))
print(f"generate, {B} questions, {max_length} new tokens: {K} beams {beam_ms:.1f} ms per batch, greedy {greedy_ms:.1f} ms per batch")

with torch.no_grad():
    rows, src, mask, pos, _, S0 = model._fewshot_prompt(b["input_ids"], emb, b["attention_mask"], shots, sentinel, max_length)
    R, E, nl, t_max, S_max = B * K, lcfg.n_embd, len(lm.layers), max_length, S0 + max_length
    drv = decode._SharedStep(lm, B, K, S0, t_max, 1)
    drv.prefill(rows, src, pos, mask)
    rep = decode._KVCache(lm, R, S_max, R)
    for l in range(nl):
        for shared, full in ((drv.cache.k[l], rep.k[l]), (drv.cache.v[l], rep.v[l])):
            full.view(R, S_max, E)[:, :S0] = shared.view(B, S0, E).repeat_interleave(K, dim=0)
    one = decode._KVCache(lm, B, S_max, B * S0)
    decode._prefill(lm, one, rows, src[:, :S0].contiguous(), pos[:, :S0].contiguous(), mask, B, S0, S_max)
    mask_r = mask.repeat_interleave(K, dim=0).contiguous()
    pos_r = pos.repeat_interleave(K, dim=0).contiguous()
    tok_r = torch.randint(3, lcfg.vocab - 8, (R,), device=dev, dtype=torch.int32)
    tok_1 = tok_r[::K].contiguous()


def replicated_step(t):
    x = ops.embed_assemble(tok_r, pos_r[:, S0 + t].contiguous(), lm.wte, None, lm.wpe)
    decode._block(lm, rep, x, mask_r, R, 1, S0 + t, S_max)
    return decode._last_logits(lm, x, R, 1)


ROUTES = {
    "shared": lambda t: drv.step(tok_r, pos_r[:, S0 + t].contiguous(), mask, t),
    "replicated": replicated_step,
    "greedy": lambda t: decode._decode_step(lm, one, tok_1, pos[:, S0 + t].contiguous(), mask, B, S0 + t, S_max),
}


def generation(step):
    marks = [ev()]
    for t in range(max_length - 1):
        step(t)
        marks.append(ev())
    torch.cuda.synchronize()
    return sum(marks[i].elapsed_time(marks[i + 1]) for i in range(len(marks) - 1)) / (len(marks) - 1)


with torch.no_grad():
    a, r = ROUTES["shared"](2), ROUTES["replicated"](2)
    torch.cuda.synchronize()
    print(f"logits of one step, shared against replicated: max |diff| {float((a - r).abs().max()):.3e} at max |logit| {float(r.abs().max()):.2f}")
    for fn in ROUTES.values():
        generation(fn)                                      # warm every shape up
    runs = {n: [] for n in ROUTES}
    for _ in range(REPS):
        for n, fn in ROUTES.items():
            runs[n].append(generation(fn))
stat = lambda xs: dict(median=float(torch.tensor(xs).median()), min=min(xs), max=max(xs))
per = {n: stat(v) for n, v in runs.items()}
diff = stat([s - q for s, q in zip(runs["shared"], runs["replicated"])])
fmt = lambda d: f"{d['median']:.3f} ms (min {d['min']:.3f}, max {d['max']:.3f})"
t_mean = (max_length - 2) / 2
kv_rep = 2 * nl * R * (S0 + t_mean + 1) * E * 2
kv_shared = 2 * nl * (B * S0 + R * (t_mean + 1)) * E * 2
weights = nl * (4 * E * E + 2 * E * lcfg.ffn) * 2
print(f"per decode step, median over {REPS} generations of {max_length - 1} steps; prompt of {S0} positions")
for n in ROUTES:
    print(f"  {n:11s} {fmt(per[n])}")
print(f"  shared - replicated, paired by generation: {fmt(diff)}")
print(f"byte model of a step (shapes, not measurements): weights {weights / 1e9:.2f} GB; K / V replicated {kv_rep / 1e9:.2f} GB, shared {kv_shared / 1e9:.2f} GB")
print(json.dumps(dict(B=B, beams=K, S0=S0, max_length=max_length, reps=REPS, beam_generate_ms=beam_ms, greedy_generate_ms=greedy_ms, step_ms=per,
                      shared_minus_replicated_ms=diff, weight_bytes=weights, kv_bytes_replicated=kv_rep, kv_bytes_shared=kv_shared)))
