#!/usr/bin/env python3
"""Answer-candidate scoring on the two few-shot shapes of the benchmark (random-init weights, bf16): T0_3B (T5 v1.1 XL) and OPT-2.7B, 32
questions with 4 shots + query (20 text tokens per segment, prefix 10: 150 prompt positions), C in {2, 16, 64} candidates of Tc = 4
tokens.

Prints ms per batch of ``score_candidates`` with ``share_prompt=True`` (the prompt encoded / prefilled once per question) and
``share_prompt=False`` (replicated per candidate: the route the shared one is compared against).  Shared and replicated calls alternate,
so that drift of the box hits both alike; per cell the median and min .. max over REPS calls after a warm-up call of each.  The CLIP
embeddings are given (no ViT encode in the brackets).  ``--only t0|opt`` restricts the models, ``--sizes 2,16`` the candidate counts,
``--shared-only`` skips the replicated route (for a kernel trace of the shared one).  The last line is one JSON object."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from eavqa_amd.data.synthetic import fewshot_batch

if not torch.cuda.is_available():
    sys.exit("score_bench.py measures on the GPU; there is none here")

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=["t0", "opt"], default=None)
ap.add_argument("--sizes", default="2,16,64")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shared-only", action="store_true")
args = ap.parse_args()

dev, dtype = "cuda:0", torch.bfloat16
B, shots, seg, L, D, TC = 32, 4, 20, 10, 768, 4
SIZES = [int(s) for s in args.sizes.split(",")]


def candidates(C, vocab, seed):
    """[B, C, TC]: 1 .. TC - 1 content tokens plus a closing token, right-padded with -100."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.full((B, C, TC), -100, dtype=torch.int64)
    n = torch.randint(1, TC, (B, C), generator=g)
    body = torch.randint(3, vocab - 200, (B, C, TC), generator=g)
    pos = torch.arange(TC)[None, None, :]
    cand = torch.where(pos < n[..., None], body, cand)
    return torch.where(pos == n[..., None], torch.ones_like(cand), cand)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(score, vocab):
    rows = {}
    for C in SIZES:
        cand = candidates(C, vocab, C)
        routes = (True,) if args.shared_only else (True, False)
        for share in routes:
            score(cand, share)                              # warm every shape up
        times = {share: [] for share in routes}
        for _ in range(args.reps):
            for share in routes:
                times[share].append(once(lambda: score(cand, share)))
        stat = lambda xs: dict(median=float(torch.tensor(xs).median()), min=min(xs), max=max(xs))
        rows[C] = {("shared" if share else "replicated"): stat(t) for share, t in times.items()}
    return rows


def report(name, rows):
    fmt = lambda d: f"{d['median']:8.2f} ms (min {d['min']:.2f}, max {d['max']:.2f})"
    print(f"{name}: {B} questions, {TC}-token candidates, ms per batch over {args.reps} calls")
    for C, r in rows.items():
        line = f"  C = {C:3d}  shared {fmt(r['shared'])}"
        if "replicated" in r:
            line += f"   replicated {fmt(r['replicated'])}   ratio {r['replicated']['median'] / r['shared']['median']:.2f}"
        print(line)


result = dict(B=B, shots=shots, Tc=TC, reps=args.reps, dtype="bf16")
torch.manual_seed(2021)
if args.only in (None, "t0"):
    from eavqa_amd.models.vct0 import VCT0Prefix
    model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version="bigscience/T0_3B", dtype=dtype, device=dev).eval()
    b = fewshot_batch(B, model.lm.cfg.vocab, shots, seg, 32099, image_size=8, device=dev)
    emb = torch.randn(B, shots + 1, D, device=dev, dtype=dtype)
    score = lambda cand, share: model.score_candidates(prefix=emb, question_tokens=b["input_ids"], question_mask=b["attention_mask"], num_shots=shots,
                                                       candidates=cand, share_prompt=share)
    result["t0_3b"] = measure(score, model.lm.cfg.vocab)
    report("T0_3B few-shot", result["t0_3b"])
    del model, score
    torch.cuda.empty_cache()
if args.only in (None, "opt"):
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import KNOWN_CONFIGS, FrozenCausalLM, LMConfig, random_init_state_dict
    lcfg = LMConfig.from_hf_dict(KNOWN_CONFIGS["facebook/opt-2.7b"])
    lm = FrozenCausalLM(lcfg, random_init_state_dict(lcfg, 2021, dev), dtype, dev)
    model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=dev).eval()
    sentinel = lcfg.vocab - 1
    b = fewshot_batch(B, lcfg.vocab, shots, seg, sentinel, image_size=8, device=dev)
    emb = torch.randn(B, shots + 1, D, device=dev, dtype=dtype)
    score = lambda cand, share: model.score_candidates_fewshot(b["input_ids"], emb, b["attention_mask"], num_shots=shots, special_token_id=sentinel,
                                                               candidates=cand, share_prompt=share)
    result["opt_2.7b"] = measure(score, lcfg.vocab)
    report("OPT-2.7B few-shot (cfg4)", result["opt_2.7b"])
print(json.dumps(result))
