#!/usr/bin/env python3
"""The Llama family as the frozen LM, random-init weights of public shapes (Llama-2-7B: multi-head; TinyLlama-1.1B: 32 heads over 4
key / value heads, expanded at load), with the OPT-6.7B leg of the same tree timed in the same process, interleaved, for scale:

  * mapper training step (forward + dgrad through the LM + mapper backward), B = 64, bf16, 10 prefix + 40 text positions per row;
  * few-shot generation, B = 32: prefill of a 150-position prompt and the cached decode step (HIP events inside greedy_decode), with
    the byte model of the step - weight bytes as streamed (grouped-query K / V rows counted expanded) plus the K / V cache read.

    python tools/llama_bench.py [--lms meta-llama/Llama-2-7b-hf,TinyLlama/TinyLlama-1.1B-Chat-v1.0,facebook/opt-6.7b] [--reps 5]
                                [--legs train,generate]

Medians over --reps interleaved repetitions.  Informative only: bench.py is the project's yardstick.
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from eavqa_amd.data.synthetic import fewshot_batch
from eavqa_amd.models.clipcap import ClipCaptionPrefix
from eavqa_amd.models.lm import KNOWN_CONFIGS, FrozenCausalLM, LMConfig, random_init_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--lms", default="meta-llama/Llama-2-7b-hf,TinyLlama/TinyLlama-1.1B-Chat-v1.0,facebook/opt-6.7b")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", default="train,generate")
a = ap.parse_args()
dev, dtype = "cuda:0", torch.bfloat16
L, D = 10, 768
names = a.lms.split(",")
legs = a.legs.split(",")

models = {}
for name in names:
    cfg = LMConfig.from_hf_dict(KNOWN_CONFIGS[name])
    lm = FrozenCausalLM(cfg, random_init_state_dict(cfg, 2021, dev), dtype, dev)
    torch.manual_seed(2021)
    models[name] = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=dev)


def weight_bytes(cfg):
    """Bytes of Linear weights one decode step streams (bf16): the layers as packed (QKV [3E, E] whatever the checkpoint's K / V heads)
    and the lm_head."""
    E, F = cfg.n_embd, cfg.ffn
    ffn = 3 * E * F if cfg.arch == "llama" else 2 * E * F
    return 2.0 * (cfg.n_layer * (4 * E * E + ffn) + E * cfg.vocab)


def train_step(model, batch):
    model.clip_project.zero_grad(set_to_none=True)
    out = model(question_tokens=batch["ids"], prefix=batch["prefix"], question_mask=batch["mask"], labels=batch["labels"])
    out.loss.backward()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if "train" in legs:
    B, T = 64, 40
    batches = {}
    for name, model in models.items():
        V = model.gpt.cfg.vocab
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(3, V - 2, (B, T), generator=g)
        batches[name] = dict(ids=ids.to(dev), mask=torch.ones(B, T, dtype=torch.long, device=dev), labels=ids.to(dev),
                             prefix=torch.randn(B, D, generator=g).to(dev))
        model.train()
        for _ in range(2):
            train_step(model, batches[name])
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(a.reps):
        for name, model in models.items():
            times[name].append(timed(lambda: train_step(model, batches[name])))
    for name in names:
        cfg, ms = models[name].gpt.cfg, statistics.median(times[name])
        rows = B * (L + T)
        flops = 2.0 * 2.0 * rows * (weight_bytes(cfg) / 2.0 - cfg.n_embd * cfg.vocab) + 2.0 * 2.0 * B * T * cfg.n_embd * cfg.vocab
        print(f"train    {name:40s} B={B} rows={rows}: {ms:8.2f} ms/step = {B / ms * 1e3:7.1f} samples/s; LM GEMMs (forward + dgrad) "
              f"{flops / ms / 1e9:7.1f} TFLOP/s = {flops / ms / 1e9 / 2500:.3f} of 2.5 PF   (min {min(times[name]):.2f} max {max(times[name]):.2f})", flush=True)

if "generate" in legs:
    B, shots, seg, new = 32, 4, 20, 10
    S0 = (shots + 1) * (1 + seg) + (L - 1) * (shots + 1)
    runs = {}
    for name, model in models.items():
        V = model.gpt.cfg.vocab
        model.eval()
        b = fewshot_batch(B, V, shots, seg, V - 1, image_size=32, device=dev)
        emb = torch.randn(B, shots + 1, D, device=dev)
        runs[name] = (lambda model=model, b=b, emb=emb, V=V: lambda marks=None: model.generate_fewshot(
            b["input_ids"], emb, b["attention_mask"], num_shots=shots, special_token_id=V - 1, max_length=new, pad_token_id=1, eos_token_id=None,
            marks=marks))()
        runs[name](); torch.cuda.synchronize()
    pre, dec = {n: [] for n in names}, {n: [] for n in names}
    for _ in range(a.reps):
        for name in names:
            marks = [("start", None)]
            e0 = torch.cuda.Event(enable_timing=True); e0.record()
            runs[name](marks); torch.cuda.synchronize()
            ev = dict(marks[1:])
            pre[name].append(e0.elapsed_time(ev["prefill"]))
            dec[name].append(ev["prefill"].elapsed_time(ev["decode"]))
    steps = new - 1
    for name in names:
        cfg = models[name].gpt.cfg
        E, NL = cfg.n_embd, cfg.n_layer
        wb = weight_bytes(cfg)
        kvb = sum(2.0 * NL * B * (S0 + t + 1) * E * 2 for t in range(steps)) / steps
        ms = statistics.median(dec[name]) / steps
        print(f"generate {name:40s} B={B} S0={S0}: mapper + prefill {statistics.median(pre[name]):7.2f} ms, decode {ms:.3f} ms/step; "
              f"{wb / 1e9:.2f} GB weights + {kvb / 1e9:.2f} GB K/V per step = {(wb + kvb) / ms / 1e9:.2f} TB/s = {(wb + kvb) / ms / 1e9 / 8:.3f} of 8 TB/s"
              f"   (step min {min(dec[name]) / steps:.3f} max {max(dec[name]) / steps:.3f})", flush=True)
