"""Generates tests/golden/constrained.npz: generation inside a closed answer set, as HF does it with ``prefix_allowed_tokens_fn``
(``PrefixConstrainedLogitsProcessor``, transformers 5.15) driven by the callback of tests/_constrained_ref.py:
  * T5: the REFERENCE's own ``VCT0Prefix.generate(..., prefix_allowed_tokens_fn=fn)`` (src/models/vct0.py:462-464 forwards it to
    ``lm.generate``) on the two tiny T5 models whose weights tests/golden/vct0_t0.npz / vct0_t5v10.npz hold, interleaved few-shot path;
  * causal: HF ``generate(inputs_embeds=[mapper(prefix) | wte(tokens)], prefix_allowed_tokens_fn=fn)`` on the tiny GPT-2 and OPT of
    tests/golden/clipcap_gpt2_mlp.npz / clipcap_opt_mlp.npz (as make_golden_causal_beam.py; ``input_ids`` start empty there).
Run on the CPU where the reference checkout and transformers are installed:

    python tests/golden/make_golden_constrained.py [output directory]

Per model the cases of ``CASES``.  A set is drawn by seed from ``TEMPLATE``: up to 12 members of 1-4 ids that share stems, with a strict
prefix pair ("new" / "new york"), members that repeat an id (so that ``repetition_penalty`` acts) and members of every length.  Inputs
and sets are re-drawn, seeds from 100 upwards, until
  * the ranking margin over FINITE values is >= 1e-3 at every arg-max of an unfinished row (greedy, from the processed scores HF
    returns) and at every ``torch.topk`` inside ``generate`` (``make_golden_beam.TopkGaps``, which skips -inf and -1e9 entries);
  * every returned ``sequences_scores`` entry is finite;
  * ``rp`` cases (sets from ``RP_TEMPLATE``): the ids (with beams: or the scores) differ from the same call without
    ``repetition_penalty``; ``cut`` cases: some returned row holds no eos.
tests/test_constrained_cpu.py recomputes membership, finiteness and the margin from the committed arrays.  The file holds data only."""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _constrained_ref as ref  # noqa: E402
from make_golden_beam import TopkGaps  # noqa: E402

MARGIN = 1e-3
PAD = -100
WIDTH = 4
# members as symbols; a set of n members is the first n.  [0] / [0, 1] / [0, 1, 2]: strict prefixes; [4, 4, 5, 6], [10, 11, 10]: repeats
TEMPLATE = [[0], [0, 1], [0, 1, 2], [0, 3], [4], [4, 4, 5, 6], [7, 8], [7, 9], [10, 11, 10], [12], [12, 13, 14, 15], [16, 17]]
SHORT = [[0], [0, 1, 2]]
# the ``rp`` cases: nearly every continuation repeats an id, so that the penalty changes a choice on most inputs
RP_TEMPLATE = [[0], [0, 0], [0, 0, 1], [0, 1], [2], [2, 2], [2, 3, 2], [3, 3], [3], [4, 4, 4, 4], [4, 5], [5, 5]]
# name, num_beams, num_return_sequences, generated positions, members per item (one number: a shared set), repetition_penalty, condition
CASES = [
    ("g_shared", 1, 1, 6, 12, 1.0, None),
    ("g_item", 1, 1, 6, (12, 7, 5), 1.0, None),
    ("b4_shared", 4, 4, 6, 12, 1.0, None),
    ("b4_item", 4, 4, 6, (12, 7, 5), 1.0, None),
    ("b4_short", 4, 2, 6, (6, 2, 6), 1.0, None),
    ("g_rp", 1, 1, 6, 12, 1.7, "rp"),
    ("b4_rp", 4, 4, 6, 12, 1.7, "rp"),
    ("g_cut", 1, 1, 2, 12, 1.0, "cut"),
    ("b4_cut", 4, 4, 2, 12, 1.0, "cut"),
]


def draw_set(gen, V, banned, n, template):
    ids = [t for t in (torch.randperm(V - 10, generator=gen) + 2).tolist() if t not in banned]
    assert len(ids) >= 18, "the vocabulary is too small for the template"
    return [[ids[s] for s in m] for m in (SHORT if n == 2 else template[:n])]


def draw_sets(seed, V, banned, case, B):
    gen = torch.Generator().manual_seed(1000 + seed)
    sizes, template = case[4], RP_TEMPLATE if case[6] == "rp" else TEMPLATE
    if isinstance(sizes, int):
        return draw_set(gen, V, banned, sizes, template), None
    return None, [draw_set(gen, V, banned, n, template) for n in sizes[:B]]


def pack_sets(shared, per_item):
    sets = [shared] if per_item is None else per_item
    out = np.full((len(sets), max(len(s) for s in sets), WIDTH), PAD, dtype=np.int64)
    for i, st in enumerate(sets):
        for j, m in enumerate(st):
            out[i, j, :len(m)] = m
    return out


def greedy_gap(scores, generated, eos):
    gap = float("inf")
    for j, s in enumerate(scores):
        alive = ~(generated[:, :j] == eos).any(dim=1)
        top = torch.sort(s.float(), dim=-1, descending=True).values[alive, :2]
        d = (top[:, 0] - top[:, 1])
        d = d[torch.isfinite(d)]
        if d.numel():
            gap = min(gap, float(d.min()))
    return gap


def run(generate, case, eos, start, shared, per_item):
    """``generate(extra)``: the model call with the case's inputs.  Returns (arrays, ok)."""
    name, k, nrs, n_new, sizes, rp, cond = case
    fn = ref.allowed_fn(eos, start, shared, per_item)
    base = dict(num_beams=k, do_sample=False, output_scores=True, return_dict_in_generate=True, prefix_allowed_tokens_fn=fn)
    if k > 1:
        base.update(num_return_sequences=nrs)
    extra = dict(repetition_penalty=rp) if rp != 1.0 else {}
    with torch.no_grad(), TopkGaps() as gaps:
        o = generate(dict(base, **extra))
    gap = gaps.min_gap
    seq = o.sequences
    if k == 1:
        gap = min(gap, greedy_gap(o.scores, seq[:, start:], eos))
    ok = gap >= MARGIN
    arrays = dict(sequences=seq.numpy(), min_gap=np.array(gap, dtype=np.float64))
    if k > 1:
        ok = ok and bool(torch.isfinite(o.sequences_scores).all())
        arrays["sequences_scores"] = o.sequences_scores.numpy()
    if cond == "rp":
        with torch.no_grad():
            plain = generate(base)
        same = plain.sequences.shape == seq.shape and torch.equal(plain.sequences, seq)
        ok = ok and not (same and (k == 1 or torch.equal(plain.sequences_scores, o.sequences_scores)))
    if cond == "cut":
        ok = ok and bool((~(seq[:, start:] == eos).any(dim=1)).any())
    # what the fixture promises, checked where it is written too
    sets = ref.item_sets(shared, per_item, seq.shape[0])
    for r, row in enumerate(seq.tolist()):
        body = ref.cut(row, eos, start)
        full = eos in row[start:]
        assert any((m == body) if full else (m[:len(body)] == body) for m in sets[r]), (name, row)
    return arrays, ok


def t5_models(tmp):
    from make_golden_beam import build_models, call_kwargs, draw_inputs
    for tag, (model, V, D) in build_models(tmp).items():
        def setup(seed, case, model=model, V=V, D=D):
            inputs = draw_inputs(seed, V, D)
            kw = call_kwargs("fs", *inputs)
            eos, B = 1, inputs[0].shape[0]
            shared, per_item = draw_sets(seed, V, {0, 1} | set(range(V - 8, V)), case, B)
            gen = lambda extra: model.generate(**kw, max_length=case[3] + 1, **extra)
            arrays = dict(tokens=inputs[0].numpy(), mask=inputs[1].numpy(), prefix=inputs[2].numpy())
            return gen, eos, 0, 1, shared, per_item, arrays                  # pad 0; the history starts behind the decoder start token
        yield tag, setup


def causal_models():
    from make_golden_causal_beam import build, draw_inputs, prompt
    for arch in ("gpt2", "opt"):
        lm, mapper, V, L, D, pad, z = build(arch)
        eos = int(lm.config.eos_token_id)

        def setup(seed, case, lm=lm, mapper=mapper, V=V, L=L, D=D, pad=pad, eos=eos):
            q, qm, p = draw_inputs(seed, V, D, False)
            with torch.no_grad():
                emb, am = prompt(lm, mapper, L, q, qm, p)
            shared, per_item = draw_sets(seed, V, {eos, pad} | set(range(V - 8, V)), case, q.shape[0])
            gen = lambda extra: lm.generate(inputs_embeds=emb, attention_mask=am, max_new_tokens=case[3], eos_token_id=eos, pad_token_id=pad, **extra)
            return gen, eos, pad, 0, shared, per_item, dict(tokens=q.numpy(), mask=qm.numpy(), prefix=p.numpy())
        yield arch, setup


def main(out_dir=HERE):
    tmp = tempfile.mkdtemp(prefix="eavqa_constrained_")
    out = {}
    try:
        families = [("t5", list(t5_models(tmp))), ("causal", list(causal_models()))]
        for family, models in families:
            for tag, setup in models:
                for case in CASES:
                    found = None
                    for seed in range(100, 400):
                        gen, eos, pad, start, shared, per_item, arrays = setup(seed, case)
                        got, ok = run(gen, case, eos, start, shared, per_item)
                        if ok:
                            found = dict(arrays, **got, sets=pack_sets(shared, per_item),
                                         params=np.array([case[1], case[2], case[3], eos, pad, 0 if per_item is None else 1], dtype=np.int64),
                                         repetition_penalty=np.array(case[5], dtype=np.float64))
                            break
                    assert found, f"{tag} {case[0]}: no seed in 100..399 satisfies the conditions"
                    print(f"{tag:6s} {case[0]:10s} seed {seed} min gap {float(found['min_gap']):.2e} sequences {found['sequences'].shape}")
                    out.update({f"{tag}.{case[0]}.{k}": v for k, v in found.items()})
        out["cases"] = np.array([c[0] for c in CASES])
        out["t5"] = np.array([t for t, _ in families[0][1]])
        out["causal"] = np.array([t for t, _ in families[1][1]])
        path = os.path.join(out_dir, "constrained.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(*sys.argv[1:2])
