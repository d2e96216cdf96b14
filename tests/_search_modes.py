"""The grid of generation modes tests/golden/search_modes.npz records (written by tests/golden/make_golden_search.py) and
tests/test_search_modes_gpu.py replays: both LM families, every step source of the pick loop, greedy / one draw / three draws per item,
plain, with rules (``repetition_penalty`` plus ``allowed_sequences``) and with ``output_scores``, and one 2-beam call per family.
fp32 on the tiny committed weights only; B = 3 items, ``max_length`` = 6."""
import functools
import json
import os

import numpy as np
import torch

from conftest import GOLDEN, load_golden

DEV = "cuda"
B, MAX_LENGTH = 3, 6
SAMPLING = dict(do_sample=True, seed=1234, top_k=5, temperature=0.8)
DRAWS = dict(seed=1234, top_k=5, temperature=0.8, num_return_sequences=3)
RULES = dict(repetition_penalty=1.3)
T5_TAGS = ("t0", "t5v10")
CAUSAL = {"gpt2": "hf_gpt2_tiny", "opt": "hf_opt_tiny"}
CAUSAL_PAD = 0
T = torch.from_numpy


def answer_set(V, seed):
    """Seven members of one to four ids that share stems and repeat an id (so that the repetition penalty acts); ids 0..2 (T5's start / pad
    and eos, OPT's pad and eos) and the last ten of the vocabulary (GPT-2's eos, the sentinels) stay out."""
    g = torch.Generator().manual_seed(seed)
    a, b, c, d, e, h = (torch.randperm(V - 13, generator=g) + 3).tolist()[:6]
    return [[a], [a, b], [a, b, c], [a, d], [e], [e, e, h, a], [h, b]]


@functools.lru_cache(maxsize=None)
def t5_model(tag):
    """(VCT0Prefix on the GPU, the prefix-only call - the input form on which greedy search leaves the start / pad id on both tiny
    models -, the decoder-prompt call with a 2-token left-padded prompt, config eos id, V)."""
    from eavqa_amd.models.t5 import FrozenT5, T5Config
    from eavqa_amd.models.vct0 import VCT0Prefix
    z = load_golden(f"vct0_{tag}.npz")
    V, E, DKV, H, F, NL, L, D, gated, tied = [int(v) for v in z["cfg"]]
    lm = FrozenT5(T5Config(E, DKV, H, F, NL, NL, V, bool(gated), bool(tied)), {n[3:]: T(v) for n, v in z.items() if n.startswith("lm.")},
                  torch.float32, DEV)
    model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=torch.float32, device=DEV).eval()
    model.clip_project.load_state_dict({n[4:]: T(v) for n, v in z.items() if n.startswith("map.")})
    plain = dict(prefix=T(z["prefix"]))
    g = torch.Generator().manual_seed(17)
    prompt = torch.randint(3, V - 10, (B, 2), generator=g)
    pmask = torch.ones_like(prompt)
    prompt[0::2, 0], pmask[0::2, 0] = lm.cfg.pad_token_id, 0                    # left padding (pad id = decoder start id) on rows 0 and 2
    dp = dict(prefix=T(z["fs_prefix"]), question_tokens=T(z["dp_tokens"]), question_mask=T(z["dp_mask"]), special_token_id=V - 1,
              decoder_input_ids=prompt, decoder_attention_mask=pmask)
    return model, plain, dp, lm.cfg.eos_token_id, V


@functools.lru_cache(maxsize=None)
def causal_model(arch):
    """(ClipCaptionPrefix over the tiny HF directory with a mapper drawn by seed on the host, the plain call, the few-shot call with two
    images per row, config eos id, V)."""
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    path = os.path.join(GOLDEN, CAUSAL[arch])
    with open(os.path.join(path, "config.json")) as f:
        V = int(json.load(f)["vocab_size"])
    L, D = 3, 16
    model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version=path, dtype=torch.float32, device=DEV).eval()
    g = torch.Generator().manual_seed(5)
    model.clip_project.load_state_dict({n: 0.3 * torch.randn(p.shape, generator=g) for n, p in model.clip_project.state_dict().items()})
    special, n_img = V - 5, 2
    tok = torch.randint(3, special - n_img - 1, (B, 9), generator=g)
    mask = torch.ones(B, 9, dtype=torch.long)
    mask[1, -2:] = 0
    plain = dict(question_tokens=tok, prefix=torch.randn(B, D, generator=g), question_mask=mask)
    tok_fs = tok.clone()
    for b in range(B):
        for i in range(n_img):
            tok_fs[b, 4 * i + (b % 2)] = special - i
    few = dict(question_tokens=tok_fs, prefix=torch.randn(B, n_img, D, generator=g), question_mask=mask, num_shots=n_img - 1,
               special_token_id=special)
    return model, plain, few, model.gpt.cfg.eos_token_id, V


def _t5_cases(tag):
    picks = {"greedy": {}, "sample1": SAMPLING, "sample3": dict(SAMPLING, num_return_sequences=3)}
    steps = {"native": (True, True), "python": (True, False), "reforward": (False, True)}
    modes = [(f"{p}.{s}", "plain", picks[p], *steps[s]) for p in picks for s in steps]
    modes += [(f"{p}.prompt", "dp", picks[p], True, True) for p in ("greedy", "sample1")]
    out = [(f"t5.{tag}.{m}.{v}", (tag, call, kw, use_cache, native, v)) for m, call, kw, use_cache, native in modes
           for v in ("plain", "rules", "scores")]
    return out + [(f"t5.{tag}.beam2.{s}.plain", (tag, "plain", dict(num_beams=2), s == "cached", True, "beam")) for s in ("cached", "reforward")]


def _causal_cases(arch):
    out = []
    for cache in ("cached", "reforward"):
        for entry in ("generate", "generate_sampled", "generate_fewshot", "generate_draws", "generate_draws_fewshot"):
            # the draws always return their scores: they have no separate `scores` variant
            for v in ("plain", "rules") + (("scores",) if "draws" not in entry else ()):
                out.append((f"{arch}.{entry}.{cache}.{v}", (arch, entry, cache == "cached", v)))
        out.append((f"{arch}.generate_beams.{cache}.plain", (arch, "generate_beams", cache == "cached", "plain")))
    return out


def cases():
    """{name: spec} of the whole grid, in a fixed order."""
    out = []
    for tag in T5_TAGS:
        out += _t5_cases(tag)
    for arch in CAUSAL:
        out += _causal_cases(arch)
    return dict(out)


def run(name, eos=None):
    """One case of :func:`cases` with ``eos_token_id=eos`` (None: the config's): ``dict(ids=int64 [rows, length][, scores=float32])``."""
    spec = cases()[name]
    if name.startswith("t5."):
        tag, call, kw, use_cache, native, variant = spec
        model, plain, dp, cfg_eos, V = t5_model(tag)
        kw = dict(plain if call == "plain" else dp, max_length=MAX_LENGTH, use_cache=use_cache, eos_token_id=cfg_eos if eos is None else eos, **kw)
        if variant == "rules":
            kw.update(RULES, allowed_sequences=answer_set(V, 3))
        model.lm.native_step = native
        try:
            if variant in ("scores", "beam"):
                o = model.generate(output_scores=True, return_dict_in_generate=True, **kw)
                scores = o.sequences_scores if variant == "beam" else torch.stack(list(o.scores))
                return dict(ids=o.sequences.numpy(), scores=scores.numpy())
            return dict(ids=model.generate(**kw).numpy())
        finally:
            model.lm.native_step = True
    arch, entry, use_cache, variant = spec
    model, plain, few, cfg_eos, V = causal_model(arch)
    kw = dict(few if "fewshot" in entry else plain, max_length=MAX_LENGTH, pad_token_id=CAUSAL_PAD, use_cache=use_cache,
              eos_token_id=cfg_eos if eos is None else eos)
    if variant == "rules":
        kw.update(RULES, allowed_sequences=answer_set(V, 3))
    if entry == "generate_sampled":                                            # one draw per row over the per-row cache
        entry, kw = "generate", dict(kw, **SAMPLING)
    if entry == "generate_beams":
        o = model.generate_beams(num_beams=2, **kw)
    elif "draws" in entry:
        o = getattr(model, entry)(**DRAWS, **kw)
    elif variant == "scores":
        ids, logp = getattr(model, entry)(output_scores=True, **kw)
        return dict(ids=np.asarray(ids, dtype=np.int64), scores=logp.numpy())
    else:
        return dict(ids=np.asarray(getattr(model, entry)(**kw), dtype=np.int64))
    return dict(ids=np.asarray(o.sequences, dtype=np.int64), scores=o.sequences_scores.numpy())


def pack(results):
    """``{name: dict(eos, stable, ids[, scores])}`` as a handful of arrays (an .npz entry per case would cost more than its data)."""
    names = list(results)
    shape3 = lambda a: list(a.shape) + [1] * (3 - a.ndim)
    ids = [results[n]["ids"] for n in names]
    scores = [results[n].get("scores", np.zeros((0,), np.float32)) for n in names]
    return dict(cases=np.array(names), eos=np.array([results[n]["eos"] for n in names], np.int64),
                stable=np.array([results[n]["stable"] for n in names], np.bool_),
                ids_shape=np.array([a.shape for a in ids], np.int64), ids=np.concatenate([a.reshape(-1) for a in ids]).astype(np.int32),
                scores_shape=np.array([shape3(a) for a in scores], np.int64), scores_ndim=np.array([a.ndim for a in scores], np.int64),
                has_scores=np.array(["scores" in results[n] for n in names], np.bool_),
                scores=np.concatenate([a.reshape(-1) for a in scores]).astype(np.float32))


def unpack(z):
    """The inverse of :func:`pack`."""
    out, i, j = {}, 0, 0
    for c, name in enumerate(str(n) for n in z["cases"]):
        ni, ns = int(np.prod(z["ids_shape"][c])), int(np.prod(z["scores_shape"][c]))
        r = dict(eos=int(z["eos"][c]), stable=bool(z["stable"][c]), ids=z["ids"][i:i + ni].astype(np.int64).reshape(z["ids_shape"][c]))
        if z["has_scores"][c]:
            r["scores"] = z["scores"][j:j + ns].reshape(z["scores_shape"][c][:int(z["scores_ndim"][c])])
        out[name] = r
        i, j = i + ni, j + ns
    return out
