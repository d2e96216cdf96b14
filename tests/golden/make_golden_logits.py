"""Generates tests/golden/vct0_logits.npz: outputs of the REFERENCE's own ``VCT0Prefix.generate(**kwargs)`` (src/models/vct0.py:396-491 ->
HF ``lm.generate``, transformers 5.15) under HF's logits processors - ``repetition_penalty``, ``no_repeat_ngram_size``, ``min_length``,
``min_new_tokens``, ``bad_words_ids`` - on the two tiny T5 models whose weights tests/golden/vct0_t0.npz / vct0_t5v10.npz already hold.
Run where the reference checkout and transformers are installed:

    python tests/golden/make_golden_logits.py [output directory]

Per model nine cases (``CASES``): seven greedy ones and two beam searches on the interleaved few-shot path (``max_length`` 10, 8 with
beams), one greedy prefix-only case.  Inputs are drawn by seed (``make_golden_beam.draw_inputs``), from 100 upwards, until
  * the ranking margin is >= 1e-3 at every arg-max of a row that has not finished (from the PROCESSED scores HF returns) and at every
    ``torch.topk`` inside ``generate`` (``make_golden_beam.TopkGaps``) - the fixture must pin the rules, not rounding;
  * the output differs from the same call without the processor arguments (plain ``repetition_penalty`` changes nothing on a few seeds).
Cases that hold eos back take as eos a token the model really emits early in the call without processors (so that the rule acts); the
bad words of ``g_bad`` are taken from that call's output too: the single-token word is the first generated token that is neither pad nor
the config's eos, the two-token word the first such adjacent pair generated under that ban.  The smallest margin is stored with every case.
tests/test_logits_plan_cpu.py recomputes the conditions from the committed arrays.  The file holds data only."""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_beam import TopkGaps, build_models, call_kwargs, draw_inputs  # noqa: E402

MARGIN = 1e-3
# name, path, num_beams, max_length, processor arguments ("eos": an early-emitted token is searched; "words": see the module docstring)
CASES = [
    ("g_rp", "fs", 1, 10, dict(repetition_penalty=1.5)),
    ("g_ng2", "fs", 1, 10, dict(no_repeat_ngram_size=2)),
    ("g_ng1", "fs", 1, 10, dict(no_repeat_ngram_size=1)),
    ("g_minlen", "fs", 1, 10, dict(min_length=8, eos=True)),
    ("g_bad", "fs", 1, 10, dict(words=True)),
    ("g_all", "fs", 1, 10, dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4, eos=True)),
    ("b_rp_ng", "fs", 3, 8, dict(repetition_penalty=1.3, no_repeat_ngram_size=2)),
    ("b_minlen", "fs", 3, 8, dict(min_length=7, eos=True)),
    ("p_ng2", "prefix", 1, 10, dict(no_repeat_ngram_size=2)),
]


def generate(model, kw, k, max_length, eos, extra):
    args = dict(kw, max_length=max_length, do_sample=False, num_beams=k, output_scores=True, return_dict_in_generate=True, **extra)
    if k > 1:
        args["num_return_sequences"] = k
    if eos is not None:
        args["eos_token_id"] = eos
    with torch.no_grad(), TopkGaps() as gaps:
        o = model.generate(**args)
    gap = gaps.min_gap
    if k == 1:                                                     # greedy: the arg-max margins of unfinished rows, from the processed scores
        end = 1 if eos is None else eos
        for j, s in enumerate(o.scores):
            alive = ~(o.sequences[:, 1:1 + j] == end).any(dim=1)
            top = torch.sort(s.float(), dim=-1, descending=True).values[alive, :2]
            if top.numel():
                gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    return o, gap


def run_case(model, case, inputs):
    name, path, k, max_length, spec = case
    kw = call_kwargs(path, *inputs)
    base, base_gap = generate(model, kw, k, max_length, None, {})
    eos_cands = [None]
    if spec.get("eos"):
        eos_cands = list(dict.fromkeys(int(t) for t in base.sequences[:, 1:max_length - 1].flatten().tolist() if int(t) > 1))
    for eos in eos_cands:
        extra = {n: v for n, v in spec.items() if n not in ("eos", "words")}
        plain, plain_gap = (base, base_gap) if eos is None else generate(model, kw, k, max_length, eos, {})
        words = []
        if spec.get("words"):
            first = next((int(t) for t in plain.sequences[:, 1:].flatten().tolist() if int(t) > 1), None)
            if first is None:
                continue
            words = [[first]]
            mid, _ = generate(model, kw, k, max_length, eos, dict(bad_words_ids=words))
            pairs = torch.stack([mid.sequences[:, 1:-1], mid.sequences[:, 2:]], dim=-1).reshape(-1, 2).tolist()
            pair = next(([int(a), int(b)] for a, b in pairs if a > 1 and b > 1), None)
            if pair is None:
                continue
            words.append(pair)
            extra["bad_words_ids"] = words
        o, gap = generate(model, kw, k, max_length, eos, extra)
        same = o.sequences.shape == plain.sequences.shape and torch.equal(o.sequences, plain.sequences)
        if gap >= MARGIN and not same:
            bw = np.full((len(words), 2), -1, dtype=np.int64)
            for i, w in enumerate(words):
                bw[i, :len(w)] = w
            arrays = dict(tokens=inputs[0].numpy(), mask=inputs[1].numpy(), prefix=(inputs[3] if path == "prefix" else inputs[2]).numpy(),
                          params=np.array([k, max_length, -1 if eos is None else eos, extra.get("no_repeat_ngram_size", 0),
                                           extra.get("min_length", 0), extra.get("min_new_tokens", 0)], dtype=np.int64),
                          repetition_penalty=np.array(extra.get("repetition_penalty", 1.0), dtype=np.float64), bad_words=bw,
                          sequences=o.sequences.numpy(), plain=plain.sequences.numpy(), min_gap=np.array(gap, dtype=np.float64))
            if k > 1:
                arrays["sequences_scores"] = o.sequences_scores.numpy()
            return eos, arrays
    return None


def main(out_dir=HERE):
    tmp = tempfile.mkdtemp(prefix="eavqa_logits_")
    out = {}
    try:
        for tag, (model, V, D) in build_models(tmp).items():
            for case in CASES:
                found = None
                for seed in range(100, 200):
                    found = run_case(model, case, draw_inputs(seed, V, D))
                    if found:
                        break
                assert found, f"{tag} {case[0]}: no seed in 100..199 satisfies the conditions"
                eos, arrays = found
                print(f"{tag:6s} {case[0]:9s} seed {seed} eos {eos} min gap {float(arrays['min_gap']):.2e} sequences {arrays['sequences'].shape}")
                out.update({f"{tag}.{case[0]}.{k}": v for k, v in arrays.items()})
        out["cases"] = np.array([c[0] for c in CASES])
        out["paths"] = np.array([c[1] for c in CASES])
        path = os.path.join(out_dir, "vct0_logits.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(*sys.argv[1:2])
