"""Generates tests/golden/vct0_beam.npz: beam-search outputs of the REFERENCE's own ``VCT0Prefix.generate(..., num_beams=k)``
(src/models/vct0.py:396-491 -> HF ``GenerationMixin._beam_search``, transformers 5.15) on the two tiny T5 models whose weights
tests/golden/vct0_t0.npz / vct0_t5v10.npz already hold.  Run where the reference checkout and transformers are installed:

    python tests/golden/make_golden_beam.py

Per model seven cases (``CASES``): the interleaved few-shot path under three (num_beams, length_penalty, early_stopping) settings with
every hypothesis returned, one with ``num_return_sequences=1``, one ``early_stopping="never"``, the prefix-only and the text-only path.
Inputs are drawn by seed (prefixes 3 * randn) and the eos id is taken from the tokens the model emits at the first positions, until every
condition below holds - the fixture must pin the SEARCH, not rounding:
  * ranking margin >= 1e-3 at every ``torch.topk`` call inside ``generate`` (smallest gap between adjacent values among the selected
    ones and the first one not selected, -1e9 sentinels ignored), for every case;  the project's fp32 logits parity is 2e-5, seven
    accumulated steps stay an order of magnitude below;
  * (the three few-shot settings, required) a step whose parent vector is not the identity ("moved"), and a returned hypothesis shorter
    than max_length - 1 beside one of full length ("short": a hypothesis entered the pool by eos and stayed in it).  ONE exception,
    ``RELAXED``: (k = 4, length_penalty 2.0) on the tied-embedding model t5v10 keeps "moved" only.  A score is divided by the squared
    length there and the tiny model's log-probabilities are about -3.5 per token, so a short hypothesis never outranks the four
    full-length ones of the last step: seeds 100 .. 111 x EVERY eos id 2 .. V - 1 were tried, none returns a short hypothesis;
  * (the other four cases, preferred) the same two conditions: seeds 100 .. 139 are searched for them first, and only if none has
    them the case falls back to the margin alone;
  * (at least one case per model) the best beam differs from greedy search on the same inputs.
tests/test_beam_cpu.py recomputes "moved", "short" and "differs" from the committed arrays and asserts the required ones, so a regenerated
fixture cannot lose them silently.
The file holds data only: inputs, ``sequences``, ``sequences_scores``, ``beam_indices`` and the recorded minimum gap per case.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

MARGIN = 1e-3
MAX_LENGTH = 8
ES = {False: 0, True: 1, "never": 2}
# name, path, num_beams, length_penalty, early_stopping, num_return_sequences, conditions required beside the margin
CASES = [
    ("fs_k3", "fs", 3, 1.0, False, 3, ("moved", "short")),
    ("fs_k4_lp2", "fs", 4, 2.0, False, 4, ("moved", "short")),
    ("fs_k2_es", "fs", 2, 1.0, True, 2, ("moved", "short")),
    ("fs_k3_nrs1", "fs", 3, 1.0, False, 1, ()),
    ("fs_k3_never", "fs", 3, 1.0, "never", 3, ()),
    ("prefix_k3", "prefix", 3, 1.0, False, 3, ()),
    ("text_k3", "text", 3, 1.0, False, 3, ()),
]
RELAXED = {("t5v10", "fs_k4_lp2"): ("moved",)}          # see the module docstring
PREFERRED = ("moved", "short")


class TopkGaps:
    """Wraps ``torch.topk`` and records the smallest ranking gap seen (see the module docstring)."""

    def __init__(self):
        self.min_gap, self.calls, self._orig = float("inf"), 0, torch.topk

    def __enter__(self):
        def topk(x, k, *a, **kw):
            self.calls += 1
            n = x.shape[-1]
            v = torch.sort(x.detach().float(), dim=-1, descending=True).values[..., :min(k + 1, n)]
            real = v > -1.0e8
            gaps = (v[..., :-1] - v[..., 1:])[real[..., :-1] & real[..., 1:]]
            if gaps.numel():
                self.min_gap = min(self.min_gap, float(gaps.min()))
            return self._orig(x, k, *a, **kw)
        torch.topk = topk
        return self

    def __exit__(self, *exc):
        torch.topk = self._orig


def build_models(tmp):
    clipcap, vct0 = _import_reference()
    from transformers import T5Config, T5ForConditionalGeneration
    models = {}
    for tag in ("t0", "t5v10"):
        z = np.load(os.path.join(HERE, f"vct0_{tag}.npz"))
        V, E, DKV, H, F, NL, L, D, gated, tied = [int(v) for v in z["cfg"]]
        cfg = T5Config(vocab_size=V, d_model=E, d_kv=DKV, num_heads=H, d_ff=F, num_layers=NL, num_decoder_layers=NL, dropout_rate=0.0,
                       feed_forward_proj="gated-gelu" if gated else "relu", tie_word_embeddings=bool(tied), decoder_start_token_id=0, pad_token_id=0,
                       eos_token_id=1, relative_attention_num_buckets=32, relative_attention_max_distance=128)
        cfg._attn_implementation = "eager"
        lm = T5ForConditionalGeneration(cfg).eval()
        missing, unexpected = lm.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lm.")}, strict=False)
        assert not unexpected and all("lm_head" in m or "embed_tokens" in m for m in missing), (missing, unexpected)
        path = os.path.join(tmp, tag)
        lm.save_pretrained(path)

        class TinyVCT0(vct0.VCT0Prefix):          # the tiny vocabulary has no id 32099: sentinel i is V - 1 - i (as make_golden.vct0_golden)
            def insert_prefix_into_input(self, *a, special_token_id=32099, _V=V, **k):
                return super().insert_prefix_into_input(*a, special_token_id=special_token_id - 32099 + (_V - 1), **k)

        model = TinyVCT0(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version=path).eval()
        model.lm.config._attn_implementation = "eager"
        model.clip_project.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("map.")})
        # the rebuilt model IS the one of vct0_golden: its greedy ids on the stored few-shot inputs are the stored ones
        with torch.no_grad():
            o = model.generate(prefix=torch.from_numpy(z["fs_prefix"]), question_tokens=torch.from_numpy(z["fs_tokens"]),
                               question_mask=torch.from_numpy(z["fs_mask"]), max_length=9, do_sample=False, num_beams=1)
        assert np.array_equal(o.numpy(), z["gen_fs_ids"]), tag
        models[tag] = (model, V, D)
    return models


def draw_inputs(seed, V, D, B=3, n_img=3, Tq=12):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randint(2, V - 8, (B, Tq), generator=gen)
    for b in range(B):
        for i, pos in enumerate(sorted(torch.randperm(Tq - 3, generator=gen)[:n_img].tolist())):
            q[b, pos] = V - 1 - i
    qm = torch.ones(B, Tq, dtype=torch.long)
    qm[1, Tq - 2:] = 0
    q[1, Tq - 2:] = 0
    pf = 3.0 * torch.randn(B, n_img, 1, D, generator=gen)
    p0 = 3.0 * torch.randn(B, D, generator=gen)
    return q, qm, pf, p0


def call_kwargs(path, q, qm, pf, p0):
    if path == "fs":
        return dict(prefix=pf, question_tokens=q, question_mask=qm)
    if path == "text":
        return dict(prefix=pf, question_tokens=q, question_mask=qm, no_prefix=True)
    return dict(prefix=p0)


def run_case(model, case, inputs, eos):
    name, path, k, lp, es, nrs, structural = case
    kw = call_kwargs(path, *inputs)
    with torch.no_grad():
        greedy = model.generate(**kw, max_length=MAX_LENGTH, do_sample=False, num_beams=1, eos_token_id=eos)
        with TopkGaps() as gaps:
            o = model.generate(**kw, max_length=MAX_LENGTH, do_sample=False, num_beams=k, num_return_sequences=nrs, length_penalty=lp,
                               early_stopping=es, eos_token_id=eos, output_scores=True, return_dict_in_generate=True)
    assert gaps.calls > 0
    bi = o.beam_indices                                            # [B * nrs, generated length], -1 after a hypothesis' end
    B = bi.shape[0] // nrs
    lens = (bi >= 0).sum(1)
    ident = torch.arange(B).repeat_interleave(nrs) * k
    # hist[:, j] = the slot a returned hypothesis' parent sat in at generation step j, which is the slot the hypothesis itself took at step
    # j - 1; a change after step 0 (where every beam descends from slot 0) is a step >= 1 whose parent vector is not the identity
    hist = bi - ident[:, None]
    moved = bool(((hist[:, 2:] != hist[:, 1:-1]) & (bi[:, 2:] >= 0)).any())
    short_and_full = bool((lens < MAX_LENGTH - 1).any() and (lens == MAX_LENGTH - 1).any())
    best = o.sequences.view(B, nrs, -1)[:, 0]
    n = min(best.shape[1], greedy.shape[1])
    differs = best.shape[1] != greedy.shape[1] or not torch.equal(best[:, :n], greedy[:, :n])
    flags = dict(margin=gaps.min_gap >= MARGIN, moved=moved, short=short_and_full, differs=differs)
    arrays = dict(tokens=inputs[0].numpy(), mask=inputs[1].numpy(), prefix=(inputs[3] if path == "prefix" else inputs[2]).numpy(),
                  params=np.array([k, nrs, ES[es], eos, MAX_LENGTH], dtype=np.int64), length_penalty=np.array(lp, dtype=np.float64),
                  sequences=o.sequences.numpy(), sequences_scores=o.sequences_scores.numpy(), beam_indices=bi.numpy().astype(np.int32),
                  min_gap=np.array(gaps.min_gap, dtype=np.float64), greedy=greedy.numpy())
    return flags, arrays


def main():
    tmp = tempfile.mkdtemp(prefix="eavqa_beam_")
    out = {}
    try:
        for tag, (model, V, D) in build_models(tmp).items():
            any_differs = False
            for case in CASES:
                found = None
                required = RELAXED.get((tag, case[0]), case[6])
                # first pass: the preferred conditions too; second pass: the required ones
                for wanted, seeds in ((tuple(set(required) | set(PREFERRED)), range(100, 140)), (required, range(100, 200))):
                    for seed in seeds:
                        inputs = draw_inputs(seed, V, D)
                        # eos: a token the model really emits early (not pad / start, not the config's eos) - row 0's greedy tokens first,
                        # then whatever a beam search without that eos puts at the first positions (the tied-embedding model's greedy rows
                        # are mostly all pad, which eos may not be)
                        with torch.no_grad():
                            kw = dict(**call_kwargs(case[1], *inputs), max_length=MAX_LENGTH, do_sample=False)
                            g = model.generate(**kw, num_beams=1)
                            bs = model.generate(**kw, num_beams=case[2], num_return_sequences=case[2])
                        cands = list(dict.fromkeys(int(t) for t in g[0, 2:5].tolist() + bs[:, 1:5].flatten().tolist() if int(t) > 1))
                        for eos in cands:
                            flags, arrays = run_case(model, case, inputs, eos)
                            if flags["margin"] and all(flags[c] for c in wanted):
                                found = (seed, eos, flags, arrays)
                                break
                        if found:
                            break
                    if found:
                        break
                assert found, f"{tag} {case[0]}: no seed in 100..199 satisfies the conditions"
                seed, eos, flags, arrays = found
                any_differs = any_differs or flags["differs"]
                print(f"{tag:6s} {case[0]:12s} seed {seed} eos {eos:3d} min gap {float(arrays['min_gap']):.2e} moved {flags['moved']} "
                      f"short {flags['short']} best != greedy {flags['differs']} sequences {arrays['sequences'].shape}")
                out.update({f"{tag}.{case[0]}.{k}": v for k, v in arrays.items()})
            assert any_differs, f"{tag}: beam search equals greedy search in every case"
        out["cases"] = np.array([c[0] for c in CASES])
        out["paths"] = np.array([c[1] for c in CASES])
        path = os.path.join(HERE, "vct0_beam.npz")
        np.savez_compressed(path, **out)
        print(f"wrote vct0_beam.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
