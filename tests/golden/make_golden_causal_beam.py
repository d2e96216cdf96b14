"""Generates tests/golden/causal_beam.npz: beam-search outputs of HF ``generate(inputs_embeds=[mapper(prefix) | wte(tokens)],
attention_mask=..., num_beams=k, max_new_tokens=n, ...)`` (``GenerationMixin._beam_search``, transformers 5.15) on the two tiny causal
LMs whose weights tests/golden/clipcap_gpt2_mlp.npz / clipcap_opt_mlp.npz already hold.  Run on the CPU where transformers is installed:

    python tests/golden/make_golden_causal_beam.py

Per model six cases (``CASES``): k in {2, 3, 4}, ``length_penalty`` 1.0 and 2.0, ``early_stopping`` False / True / "never",
``num_return_sequences`` 1 and k, one case with ``no_repeat_ngram_size=2``.  GPT-2 cases use full attention masks only: HF's ``generate``
derives GPT-2's positions from the mask, the reference's loop and this project count them with arange, so the two agree only without
padding.  OPT cases pad one row only if the first-step logits of ``generate`` on a padded prompt agree with the project's CPU oracle
(oracle/ref_cpu.py) to 2e-5, which the generator checks first; they do not (``generate`` gives the pads of a right-padded OPT prompt
position ids of its own, and the first query sits on a pad), so the OPT cases use full masks too.
Inputs are drawn by seed (prefixes 3 * randn) and the eos id is taken from the tokens the model emits at the first positions, until the
conditions hold - the fixture must pin the SEARCH, not rounding (as make_golden_beam.py):
  * ranking margin >= 1e-3 at every ``torch.topk`` call inside ``generate``, for every case;
  * (preferred per case, required once per model each) a step whose parent vector is not the identity ("moved"), a returned hypothesis
    shorter than the longest beside one of full length ("short"), a best beam that differs from greedy search ("differs").
tests/test_causal_beam_cpu.py recomputes the three conditions and the margin from the committed arrays.
The file holds data only: inputs, ``sequences``, ``sequences_scores``, ``beam_indices``, the greedy ids and the recorded minimum gap."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden_beam import TopkGaps  # noqa: E402

MARGIN = 1e-3
NEW_TOKENS = 6
B, TQ = 2, 6
ES = {False: 0, True: 1, "never": 2}
# name, num_beams, length_penalty, early_stopping, num_return_sequences, no_repeat_ngram_size
CASES = [
    ("k3", 3, 1.0, False, 3, 0),
    ("k4_lp2", 4, 2.0, False, 4, 0),
    ("k2_es", 2, 1.0, True, 2, 0),
    ("k3_nrs1", 3, 1.0, False, 1, 0),
    ("k3_never", 3, 1.0, "never", 3, 0),
    ("k3_ngram2", 3, 1.0, False, 3, 2),
]
PREFERRED = ("moved", "short")


def build(arch):
    """(HF model, mapper function, V, L, D, pad id, oracle pieces) from the fixture's arrays."""
    from transformers import GPT2Config, GPT2LMHeadModel, OPTConfig, OPTForCausalLM
    z = np.load(os.path.join(HERE, f"clipcap_{arch}_mlp.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lm.")}
    if arch == "gpt2":
        V, E, NLAY, NH, NPOS, L, D = [int(v) for v in z["cfg"][:7]]
        cfg = GPT2Config(vocab_size=V, n_embd=E, n_layer=NLAY, n_head=NH, n_positions=NPOS, activation_function="gelu_new", resid_pdrop=0.0,
                         embd_pdrop=0.0, attn_pdrop=0.0, bos_token_id=V - 1, eos_token_id=V - 1)
        lm = GPT2LMHeadModel(cfg)
    else:
        V, E, NLAY, NH, NPOS, L, D, FFN = [int(v) for v in z["cfg"]]
        cfg = OPTConfig(vocab_size=V, hidden_size=E, num_hidden_layers=NLAY, num_attention_heads=NH, max_position_embeddings=NPOS, ffn_dim=FFN,
                        word_embed_proj_dim=E, dropout=0.0, attention_dropout=0.0, activation_function="relu", pad_token_id=1, bos_token_id=2,
                        eos_token_id=2)
        lm = OPTForCausalLM(cfg)
    cfg._attn_implementation = "eager"
    missing, unexpected = lm.load_state_dict(sd, strict=False)
    assert not unexpected and all("lm_head" in m or "attn.bias" in m or "masked_bias" in m for m in missing), (missing, unexpected)
    lm.eval()
    m = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("map.")}

    def mapper(p):
        h = torch.tanh(p @ m["model.0.weight"].t() + m["model.0.bias"])
        return (h @ m["model.2.weight"].t() + m["model.2.bias"]).view(p.shape[0], L, E)

    return lm, mapper, V, L, D, int(z["pad_id"]), z


def draw_inputs(seed, V, D, padded):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randint(3, V - 8, (B, TQ), generator=gen)
    qm = torch.ones(B, TQ, dtype=torch.long)
    if padded:
        qm[1, TQ - 2:] = 0
    p = 3.0 * torch.randn(B, D, generator=gen)
    return q, qm, p


def prompt(lm, mapper, L, q, qm, p):
    emb = torch.cat([mapper(p), lm.get_input_embeddings()(q)], dim=1)
    return emb, torch.cat([torch.ones(B, L, dtype=torch.long), qm], dim=1)


def opt_padding_agrees(lm, mapper, V, L, D, z):
    """The padded prompt's first-step logits from HF against the project's float64 CPU oracle: both within 2e-5?"""
    from oracle import ref_cpu
    q, qm, p = draw_inputs(100, V, D, True)
    sd = {k[3:]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith("lm.")}
    mp = {k[4:]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith("map.")}
    cfg = dict(arch="opt", n_layer=int(z["cfg"][2]), n_head=int(z["cfg"][3]))
    with torch.no_grad():
        emb, am = prompt(lm, mapper, L, q, qm, p)
        # the first step of ``generate`` itself, not a plain forward: generate hands the model position ids of its own (pads get position 1)
        hf = lm.generate(inputs_embeds=emb, attention_mask=am, max_new_tokens=1, do_sample=False, pad_token_id=int(z["pad_id"]), eos_token_id=None,
                         output_logits=True, return_dict_in_generate=True).logits[0]
        e64, m64 = ref_cpu._prefix_inputs(sd, cfg, mp, dict(prefix_length=L, mapping_type="mlp"), q, p.double(), qm.double())
        want = ref_cpu.lm_logits(sd, cfg, e64, m64)[:, -1]
    err = float((hf.double() - want).abs().max())
    print(f"opt: padded prompt, first-step logits of HF generate against the CPU oracle: max |diff| {err:.2e}")
    return err <= 2e-5


def run_case(lm, case, emb, am, eos, pad):
    name, k, lp, es, nrs, ngram = case
    extra = dict(no_repeat_ngram_size=ngram) if ngram else {}
    common = dict(inputs_embeds=emb, attention_mask=am, max_new_tokens=NEW_TOKENS, do_sample=False, eos_token_id=eos, pad_token_id=pad, **extra)
    with torch.no_grad():
        greedy = lm.generate(**common, num_beams=1)
        with TopkGaps() as gaps:
            o = lm.generate(**common, num_beams=k, num_return_sequences=nrs, length_penalty=lp, early_stopping=es, output_scores=True,
                            return_dict_in_generate=True)
    assert gaps.calls > 0
    bi = o.beam_indices                                            # [B * nrs, generated length], -1 after a hypothesis' end
    flags = dict(structure(bi.numpy(), o.sequences.numpy(), greedy.numpy(), k, nrs), margin=gaps.min_gap >= MARGIN)
    arrays = dict(params=np.array([k, nrs, ES[es], eos, NEW_TOKENS, ngram, pad], dtype=np.int64), length_penalty=np.array(lp, dtype=np.float64),
                  sequences=o.sequences.numpy(), sequences_scores=o.sequences_scores.numpy(), beam_indices=bi.numpy().astype(np.int32),
                  min_gap=np.array(gaps.min_gap, dtype=np.float64), greedy=greedy.numpy())
    return flags, arrays


def structure(bi, sequences, greedy, k, nrs):
    """"moved" / "short" / "differs" of one case from its arrays (tests/test_causal_beam_cpu.py recomputes the same)."""
    n_items = bi.shape[0] // nrs
    lens = (bi >= 0).sum(1)
    hist = bi - (np.repeat(np.arange(n_items), nrs) * k)[:, None]
    # hist[:, j] = the slot a returned hypothesis' parent sat in at step j = the slot the hypothesis took at step j - 1; a change after
    # step 0 (where every beam descends from slot 0) is a step >= 1 whose parent vector is not the identity
    moved = bool(((hist[:, 2:] != hist[:, 1:-1]) & (bi[:, 2:] >= 0)).any())
    short = bool((lens < lens.max()).any())
    best = sequences.reshape(n_items, nrs, -1)[:, 0]
    n = min(best.shape[1], greedy.shape[1])
    differs = best.shape[1] != greedy.shape[1] or not np.array_equal(best[:, :n], greedy[:, :n])
    return dict(moved=moved, short=short, differs=bool(differs))


def main():
    out = {}
    for arch in ("gpt2", "opt"):
        lm, mapper, V, L, D, pad, z = build(arch)
        padded = arch == "opt" and opt_padding_agrees(lm, mapper, V, L, D, z)
        seen = dict(moved=False, short=False, differs=False)
        for case in CASES:
            found = None
            for wanted, seeds in ((PREFERRED, range(100, 160)), ((), range(100, 900))):
                for seed in seeds:
                    q, qm, p = draw_inputs(seed, V, D, padded)
                    with torch.no_grad():
                        emb, am = prompt(lm, mapper, L, q, qm, p)
                        kw = dict(inputs_embeds=emb, attention_mask=am, max_new_tokens=NEW_TOKENS, do_sample=False, pad_token_id=pad, eos_token_id=None)
                        g = lm.generate(**kw, num_beams=1)
                        bs = lm.generate(**kw, num_beams=case[1], num_return_sequences=case[1])
                    cands = list(dict.fromkeys(int(t) for t in g[0, 1:4].tolist() + bs[:, 1:4].flatten().tolist() + g[:, :5].flatten().tolist()
                                                + bs[:, :5].flatten().tolist() if int(t) != pad))
                    for eos in cands:
                        flags, arrays = run_case(lm, case, emb, am, eos, pad)
                        if flags["margin"] and all(flags[c] for c in wanted):
                            found = (seed, eos, flags, dict(arrays, tokens=q.numpy(), mask=qm.numpy(), prefix=p.numpy()))
                            break
                    if found:
                        break
                if found:
                    break
            assert found, f"{arch} {case[0]}: no seed in 100..899 satisfies the conditions"
            seed, eos, flags, arrays = found
            for c in seen:
                seen[c] = seen[c] or flags[c]
            print(f"{arch:5s} {case[0]:10s} seed {seed} eos {eos:3d} min gap {float(arrays['min_gap']):.2e} moved {flags['moved']} "
                  f"short {flags['short']} best != greedy {flags['differs']} sequences {arrays['sequences'].shape}")
            out.update({f"{arch}.{case[0]}.{k}": v for k, v in arrays.items()})
        assert all(seen.values()), f"{arch}: {seen}"
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, "causal_beam.npz")
    np.savez_compressed(path, **out)
    print(f"wrote causal_beam.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
