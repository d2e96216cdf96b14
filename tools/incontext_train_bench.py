#!/usr/bin/env python3
"""The mapper training step on in-context episodes (`profiles/incontext_training.md`): 4 shots + the query = 5 images per row, one
sentinel + 20 text tokens per segment, prefix length 10 -> 150 positions per row, B = 16, bf16, synthetic weights:

  t0_3b     `VCT0Model.forward(prefix, labels, question_tokens, question_mask)`: the T0_3B encoder over the 150 interleaved positions,
            the decoder teacher-forced on a 4-token answer;
  opt_1p3b  `ClipCaptionModel.forward_fewshot` on OPT-1.3B (the LM of bench.py's cfg3): the last 3 tokens of every segment are scored.

Beside each, the single-image step at the same number of attended rows (one image, 140 text tokens, the same labels per row): on the
causal path the existing `forward`, on T0 the new `forward` with one sentinel; and on T0 the caption step the project already had
(10 encoder positions per row).  A step is mapper forward (from CLIP embeddings, as the reference trains from pre-extracted ones) ->
frozen LM forward -> backward into the mapper -> fused AdamW.

Row and FLOP model: a step runs B * 150 LM rows in every variant; the frozen LM costs forward + dgrad = 2 x forward FLOPs
(2 x parameters x rows for the projections + 4 S^2 E per layer for attention, the lm_head on the scored rows only for the causal LM), the
mapper 3 x (forward, dgrad, wgrad) per image.  The episode and the single-image step differ in the mapper (5 images against 1) and in
where the prefix rows sit; the LM rows and their FLOPs are the same.

Every model runs in a child process of its own under a time limit; inside it the variants are timed with device events around whole
steps, interleaved (A, B, C, A, B, C, ...), and the medians are reported; then what differs between the episode and the single-image step
is timed alone (`parts_ms`: the mapper's forward + backward on 80 and on 16 images, the label layout).  One JSON line per model."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SHOTS, SEG, L, D = 16, 4, 20, 10, 768           # D: the ViT-L/14 projection width (cfg3 / the T0 legs of bench.py)
N_IMG = SHOTS + 1
T_EPISODE = N_IMG * (1 + SEG)                      # 105 tokens -> 150 positions
S = T_EPISODE + (L - 1) * N_IMG
ANSWER = 3                                         # scored tokens per segment (causal)
TD = 4                                             # decoder targets (T5)


def mlp_flops(E):
    H = E * L // 2
    return 2 * (D * H + H * E * L)


def causal_flops(c, n_img, scored):
    E, F, V = c.n_embd, c.ffn, c.vocab
    lm = c.n_layer * (2 * S * (4 * E * E + 2 * E * F) + 4 * S * S * E) + 2 * scored * E * V
    return 2 * lm + 3 * n_img * mlp_flops(E)


def t5_flops(c, enc_pos, n_img):
    import bench
    enc, dec = bench._t5_stack_flops(c, enc_pos, TD)
    return 2 * (enc + dec + 2 * TD * c.d_model * c.vocab) + 3 * n_img * mlp_flops(c.d_model)


def episode_tokens(vocab, special, g):
    import torch
    tok = torch.randint(3, min(vocab, special - N_IMG) - 2, (B, T_EPISODE), generator=g)
    labels = torch.full((B, T_EPISODE), -100, dtype=torch.long)
    for i in range(N_IMG):
        tok[:, i * (1 + SEG)] = special - i
        end = (i + 1) * (1 + SEG)
        labels[:, end - ANSWER:end] = tok[:, end - ANSWER:end]
    return tok, labels


def child(name, reps, warmup):
    import torch
    from eavqa_amd.trainers.optim import FusedAdamW
    dev, dtype = "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(2021)
    emb5 = torch.randn(B, N_IMG, D, generator=g).to(dev)
    emb1 = emb5[:, :1].contiguous()
    ones = lambda t: torch.ones_like(t)
    if name == "opt_1p3b":
        from eavqa_amd.models.clipcap import ClipCaptionPrefix
        from eavqa_amd.models.lm import KNOWN_CONFIGS, FrozenCausalLM, LMConfig, random_init_state_dict
        c = LMConfig.from_hf_dict(KNOWN_CONFIGS["facebook/opt-1.3b"])
        lm = FrozenCausalLM(c, random_init_state_dict(c, 2021, dev), dtype, dev)
        torch.manual_seed(2021)
        model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=dev).train()
        special = c.vocab - 1
        tok, labels = episode_tokens(c.vocab, special, g)
        tok1 = torch.randint(3, c.vocab - N_IMG - 3, (B, S - L), generator=g)          # 140 text tokens behind the prefix: 150 positions
        labels1 = torch.full_like(tok1, -100)
        labels1[:, -N_IMG * ANSWER:] = tok1[:, -N_IMG * ANSWER:]
        variants = {
            "episode": lambda: model.forward_fewshot(tok, emb5, ones(tok), labels, num_shots=SHOTS, special_token_id=special),
            "single_image": lambda: model(question_tokens=tok1, prefix=emb1[:, 0], question_mask=ones(tok1), labels=labels1),
        }
        flops = {"episode": causal_flops(c, N_IMG, N_IMG * ANSWER), "single_image": causal_flops(c, 1, N_IMG * ANSWER)}
        rows = {"episode": B * S, "single_image": B * S}
    else:
        from eavqa_amd.models.t5 import KNOWN_T5, FrozenT5, T5Config, random_init_t5_state_dict
        from eavqa_amd.models.vct0 import VCT0Prefix
        c = T5Config.from_hf_dict(KNOWN_T5["bigscience/T0_3B"])
        lm = FrozenT5(c, random_init_t5_state_dict(c, 2021, dev), dtype, dev)
        torch.manual_seed(2021)
        model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=dev).train()
        special = 32099
        tok, _ = episode_tokens(c.vocab, special, g)
        tok1 = torch.randint(3, special - N_IMG - 2, (B, S - L + 1), generator=g)      # one sentinel + 140 text tokens: 150 positions
        tok1[:, 0] = special
        labels = torch.randint(3, 32000, (B, TD), generator=g)
        labels[:, -1] = c.eos_token_id
        variants = {
            "episode": lambda: model(prefix=emb5, labels=labels, question_tokens=tok, question_mask=ones(tok), num_shots=SHOTS),
            "single_image": lambda: model(prefix=emb1, labels=labels, question_tokens=tok1, question_mask=ones(tok1), num_shots=0),
            "caption": lambda: model(prefix=emb1[:, 0], labels=labels),
        }
        flops = {"episode": t5_flops(c, S, N_IMG), "single_image": t5_flops(c, S, 1), "caption": t5_flops(c, L, 1)}
        rows = {"episode": B * S, "single_image": B * S, "caption": B * L}
    opt = FusedAdamW(model.clip_project.flat, lr=1e-4)

    def step(fn):
        loss = fn().loss
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    times = {k: [] for k in variants}
    last = {}
    for r in range(warmup + reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = step(fn)
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    out = {"model": name, "dtype": "bf16", "weights": "synthetic", "batch": B, "images_per_row": N_IMG, "positions_per_row": S, "reps": reps, "warmup": warmup}
    for k, ts in times.items():
        ms = statistics.median(ts)
        loss = float(last[k])
        assert loss == loss, f"{k}: the loss is NaN"
        out[k] = {"ms_per_step": round(ms, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "samples_per_s": round(B / ms * 1e3, 1),
                  "lm_rows": rows[k], "model_TFLOP_per_step": round(B * flops[k] * 1e-12, 3), "TFLOP_per_s": round(B * flops[k] / ms * 1e-9, 1),
                  "loss": round(loss, 4)}
    out["episode_over_single_image"] = round(out["episode"]["ms_per_step"] / out["single_image"]["ms_per_step"], 4)
    out["parts_ms"] = parts(model, emb5, emb1, tok if name == "opt_1p3b" else None, labels if name == "opt_1p3b" else None, special, opt, reps, warmup)
    print(json.dumps(out), flush=True)


def parts(model, emb5, emb1, tok, labels, special, opt, reps, warmup):
    """What differs between the episode and the single-image step, timed alone (medians, interleaved): the mapper's forward + backward on
    B * 5 and on B images, and (causal path) the label layout of the episode."""
    import torch
    from eavqa_amd import ops

    def mapper(emb):
        y = model.clip_project(emb.reshape(-1, emb.shape[-1]))
        y.backward(torch.ones_like(y))
        opt.zero_grad()

    todo = {"mapper_5_images": lambda: mapper(emb5), "mapper_1_image": lambda: mapper(emb1)}
    if tok is not None:
        tk, lb = tok.to(emb5.device), labels.to(emb5.device)
        todo["label_layout"] = lambda: ops.build_fewshot_labels(tk, lb, L, N_IMG, special)
    times = {k: [] for k in todo}
    for r in range(warmup + reps):
        for k, fn in todo.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return {k: round(statistics.median(ts), 3) for k, ts in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="t0_3b,opt_1p3b")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per model (child process)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.warmup)
    for name in args.models.split(","):
        if name not in ("t0_3b", "opt_1p3b"):
            ap.error(f"unknown model {name!r}")
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
