"""GPU: beam search and n draws per prompt on the causal path (``ClipCaptionModel.generate_beams`` / ``generate_draws`` and their few-shot
forms) on the tiny GPT-2 / OPT of clipcap_gpt2_mlp.npz / clipcap_opt_mlp.npz: the cached route (one shared prompt cache) against the
re-forward route, against HF's own beam search (tests/golden/causal_beam.npz), and against ``generate``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _causal_models as cm
from conftest import load_golden

T = torch.from_numpy
F32, BF16 = torch.float32, torch.bfloat16
ES = {0: False, 1: True, 2: "never"}


def _early_eos(model, tok, prefix, mask, pad, k=1):
    """A token the tiny model emits early, so that hypotheses finish and the pool fills: of the tokens that a search WITHOUT a reachable eos
    emits, the first one with which hypotheses of different lengths are returned (k = 1: row 0's second
    greedy token)."""
    if k == 1:
        return int(model.generate(tok, prefix, mask, max_length=3, pad_token_id=pad, eos_token_id=None)[0][1])
    free = model.generate_beams(tok, prefix, mask, num_beams=k, num_return_sequences=k, max_length=12, pad_token_id=pad, eos_token_id=pad,
                                use_cache=False)
    for eos in dict.fromkeys(t for r in free.sequences for t in r if t != pad):
        out = model.generate_beams(tok, prefix, mask, num_beams=k, num_return_sequences=k, max_length=12, pad_token_id=pad, eos_token_id=eos,
                                   use_cache=False)
        if len({len([t for t in r if t != pad]) for r in out.sequences}) > 1:
            return int(eos)
    return None                                             # short hypotheses exist but none ranks among the k best: other inputs


def _beam_inputs(model, z, B, k, pad):
    """Drawn inputs and an eos with which finished hypotheses of different lengths are returned (the first of six seeds that has one)."""
    for seed in range(40 + B, 46 + B):
        tok, mask, prefix = cm.drawn_inputs(z, B, seed)
        eos = _early_eos(model, tok, prefix, mask, pad, k)
        if eos is not None:
            return tok, mask, prefix, eos
    raise AssertionError("test input: no seed / early token returns hypotheses of different lengths")


@pytest.mark.parametrize("B,k", [(2, 4), (9, 8)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_cached_beams_equal_the_reforward_route(arch, dtype, B, k):
    z, model = cm.model(arch, dtype)
    pad = int(z["pad_id"])
    tok, mask, prefix, eos = _beam_inputs(model, z, B, k, pad)
    kw = dict(num_beams=k, num_return_sequences=k, max_length=12, pad_token_id=pad, eos_token_id=eos)
    a = model.generate_beams(tok, prefix, mask, use_cache=True, **kw)
    b = model.generate_beams(tok, prefix, mask, use_cache=False, **kw)
    lens = [len([t for t in r if t != pad]) for r in a.sequences]
    err = float((a.sequences_scores - b.sequences_scores).abs().max())
    print(f"[{arch} {dtype} B={B} k={k}] eos {eos}, hypothesis lengths {min(lens)}..{max(lens)}, max |score diff| {err:.2e}")
    assert len(a.sequences) == B * k and len({len(r) for r in a.sequences}) == 1 and a.sequences_scores.shape == (B * k,)
    assert min(lens) < max(lens)                            # the pool did fill with finished hypotheses
    assert a.sequences == b.sequences
    if dtype == F32:
        assert err <= 2e-4


@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_cached_fewshot_beams_equal_the_reforward_route(arch):
    z, model = cm.model(arch, F32)
    pad = int(z["pad_id"])
    tok, mask, prefix, n_img, special = cm.fewshot_inputs(z)
    ids = model.generate_fewshot(tok, prefix, mask, num_shots=n_img - 1, special_token_id=special, max_length=3, pad_token_id=pad, eos_token_id=None)
    kw = dict(num_shots=n_img - 1, special_token_id=special, num_beams=3, num_return_sequences=3, max_length=8, pad_token_id=pad,
              eos_token_id=int(ids[0][1]), length_penalty=1.5)
    a = model.generate_beams_fewshot(tok, prefix, mask, use_cache=True, **kw)
    b = model.generate_beams_fewshot(tok, prefix, mask, use_cache=False, **kw)
    assert a.sequences == b.sequences and float((a.sequences_scores - b.sequences_scores).abs().max()) <= 2e-4


def _fixture_cases():
    z = load_golden("causal_beam.npz")
    return [(arch, str(c)) for arch in ("gpt2", "opt") for c in z["cases"]]


@pytest.mark.parametrize("use_cache", [True, False], ids=["cached", "reforward"])
@pytest.mark.parametrize("arch,case", _fixture_cases(), ids=lambda v: str(v))
def test_beams_equal_hf_beam_search(arch, case, use_cache):
    """ids equal to HF's including shape and fill, scores within 2e-4 (fp32)."""
    f = load_golden("causal_beam.npz")
    z, model = cm.model(arch, F32)
    g = lambda n: f[f"{arch}.{case}.{n}"]
    k, nrs, es, eos, n_new, ngram, pad = [int(v) for v in g("params")]
    extra = dict(no_repeat_ngram_size=ngram) if ngram else {}
    out = model.generate_beams(T(g("tokens")), T(g("prefix")), T(g("mask")), num_beams=k, num_return_sequences=nrs,
                               length_penalty=float(g("length_penalty")), early_stopping=ES[es], max_length=n_new, pad_token_id=pad, eos_token_id=eos,
                               use_cache=use_cache, **extra)
    got = np.asarray(out.sequences)
    err = float(np.abs(out.sequences_scores.numpy() - g("sequences_scores")).max())
    print(f"[{arch} {case} cache={use_cache}] sequences {got.shape}, max |score - HF| {err:.2e} (HF min gap {float(g('min_gap')):.2e})")
    assert got.shape == g("sequences").shape and np.array_equal(got, g("sequences"))
    assert out.sequences_scores.dtype == torch.float32 and err <= 2e-4


@pytest.mark.parametrize("use_cache", [True, False], ids=["cached", "reforward"])
@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_draws_with_top_k_1_are_the_greedy_row(arch, use_cache):
    z, model = cm.model(arch, F32)
    pad, eos = int(z["pad_id"]), None
    tok, mask, prefix = cm.drawn_inputs(z, 3, 7)
    eos = _early_eos(model, tok, prefix, mask, pad)
    want = model.generate(tok, prefix, mask, max_length=8, pad_token_id=pad, eos_token_id=eos)
    out = model.generate_draws(tok, prefix, mask, num_return_sequences=4, top_k=1, seed=3, max_length=8, pad_token_id=pad, eos_token_id=eos,
                               use_cache=use_cache)
    assert out.sequences == [row for row in want for _ in range(4)]
    assert out.sequences_scores.shape == (12,) and float(out.sequences_scores.abs().max()) <= 1e-4     # p(drawn) = 1 under top_k = 1
    one = model.generate_draws(tok, prefix, mask, num_return_sequences=1, top_k=1, seed=3, max_length=8, pad_token_id=pad, eos_token_id=eos,
                               use_cache=use_cache)
    assert one.sequences == model.generate(tok, prefix, mask, max_length=8, pad_token_id=pad, eos_token_id=eos, do_sample=True, top_k=1, seed=3,
                                           use_cache=use_cache)


def test_fewshot_draws_with_top_k_1_are_the_greedy_row():
    z, model = cm.model("opt", F32)
    pad = int(z["pad_id"])
    tok, mask, prefix, n_img, special = cm.fewshot_inputs(z)
    kw = dict(num_shots=n_img - 1, special_token_id=special, max_length=6, pad_token_id=pad, eos_token_id=None)
    want = model.generate_fewshot(tok, prefix, mask, **kw)
    for use_cache in (True, False):
        out = model.generate_draws_fewshot(tok, prefix, mask, num_return_sequences=3, top_k=1, seed=1, use_cache=use_cache, **kw)
        assert out.sequences == [row for row in want for _ in range(3)]


@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_draws_follow_their_seed_and_score_their_tokens(arch):
    z, model = cm.model(arch, F32)
    pad = int(z["pad_id"])
    tok, mask, prefix = cm.drawn_inputs(z, 3, 11)
    kw = dict(num_return_sequences=5, temperature=1.3, top_k=0, max_length=8, pad_token_id=pad, eos_token_id=None)
    a = model.generate_draws(tok, prefix, mask, seed=5, **kw)
    b = model.generate_draws(tok, prefix, mask, seed=5, **kw)
    c = model.generate_draws(tok, prefix, mask, seed=6, **kw)
    slow = model.generate_draws(tok, prefix, mask, seed=5, use_cache=False, **kw)
    assert a.sequences == b.sequences and torch.equal(a.sequences_scores, b.sequences_scores)
    assert a.sequences != c.sequences
    assert len({tuple(r) for r in a.sequences[:5]}) > 1     # the draws of one question are not copies of each other
    assert a.sequences == slow.sequences and float((a.sequences_scores - slow.sequences_scores).abs().max()) <= 2e-4
    assert (a.sequences_scores < 0).all() and torch.isfinite(a.sequences_scores).all()


def test_existing_behaviour_still_holds(monkeypatch):
    z, model = cm.model("gpt2", F32)
    pad = int(z["pad_id"])
    tok, mask, prefix = T(z["gen_ids"]), T(z["gen_mask"]), T(z["prefix"])
    with pytest.raises(TypeError):
        model.generate(tok, prefix, mask, num_beams=2)
    with pytest.raises(NotImplementedError):
        model.generate(tok, prefix, mask, do_sample=True, num_return_sequences=2, pad_token_id=pad)
    want = model.generate(tok, prefix, mask, max_length=6, pad_token_id=pad)
    one = model.generate_beams(tok, prefix, mask, num_beams=1, max_length=6, pad_token_id=pad)
    assert one.sequences == want and one.sequences_scores.shape == (tok.shape[0],) and (one.sequences_scores < 0).all()
    with pytest.raises(TypeError, match="top_k"):
        model.generate_beams(tok, prefix, mask, num_beams=2, pad_token_id=pad, top_k=3)
    monkeypatch.setattr(model.gpt, "weight_format", "fp8", raising=False)
    with pytest.raises(NotImplementedError, match="fp8"):
        model.generate_beams(tok, prefix, mask, num_beams=2, pad_token_id=pad)
    with pytest.raises(NotImplementedError, match="fp8"):
        model.generate_draws(tok, prefix, mask, num_return_sequences=2, pad_token_id=pad)
