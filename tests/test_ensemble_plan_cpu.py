"""CPU: the argument rules of ensemble decoding, with no device - what ``search.ensemble_plan`` and the model entry points reject and
with which exception, the weight rule, the host-side selection of ``ensemble="select"``, and ``eavqa_ensemble_combine``'s validation
before any launch."""
from types import SimpleNamespace

import pytest
import torch

import _ensemble_ref as ref
from eavqa_amd.models import search
from eavqa_amd.models.clipcap import ClipCaptionModel
from eavqa_amd.models.vct0 import VCT0Model, generation_plan


def test_accepted_arguments_pass_both_plans():
    kw = dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=3, repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=2,
              bad_words_ids=[[5]], eos_token_id=1)
    for kind in search.ENSEMBLE_KINDS:
        assert search.ensemble_plan(kind, 4, None, kw) == dict(ensemble=kind, n=4, weights=None)
    plan = generation_plan(kw, None, max_length=6, config_eos_token_id=1)
    assert plan["do_sample"] and plan["logits"] is not None
    plan = generation_plan(dict(allowed_sequences=[[5, 6], [7]], repetition_penalty=1.3), None, max_length=6, config_eos_token_id=1)
    assert plan["constraint"] is not None
    assert search.ensemble_plan("product", 8, None, dict(num_beams=1, num_return_sequences=1, allowed_sequences=[[5]]))["n"] == 8


@pytest.mark.parametrize("kw,extra,name", [
    (dict(num_beams=2), {}, "num_beams"),
    (dict(num_return_sequences=2), {}, "num_return_sequences"),
    (dict(do_sample=True, num_return_sequences=3), {}, "num_return_sequences"),
    ({}, dict(decoder_input_ids=torch.zeros(2, 1, dtype=torch.long)), "decoder_input_ids"),
    ({}, dict(one_at_a_time=True), "pass_examples_through_encoder_one_at_a_time"),
    ({}, dict(weight_format="fp8"), "lm_weight_format"),
])
@pytest.mark.parametrize("kind", search.ENSEMBLE_KINDS)
def test_what_is_not_built_raises_naming_the_argument(kind, kw, extra, name):
    with pytest.raises(NotImplementedError, match=name):
        search.ensemble_plan(kind, 3, None, kw, **extra)


def test_more_than_eight_members_are_not_built():
    with pytest.raises(NotImplementedError, match="n=9"):
        search.ensemble_plan("product", 9, None, {})
    with pytest.raises(ValueError):
        search.ensemble_plan("product", 0, None, {})
    with pytest.raises(ValueError, match="ensemble="):
        search.ensemble_plan("average", 2, None, {})


def test_weights_are_normalised():
    assert search.ensemble_weights(None, 3) is None
    assert search.ensemble_weights([2, 6], 2) == [0.25, 0.75]
    assert search.ensemble_weights(torch.tensor([1.0, 0.0, 3.0]), 3) == [0.25, 0.0, 0.75]
    for w, n in (([1, 2, 5], 3), ([0.0, 7.0], 2), ([3.0], 1)):
        got = search.ensemble_weights(w, n)
        assert got == ref.normalise(w, n) and abs(sum(got) - 1.0) <= 1e-15
    assert search.ensemble_plan("mixture", 2, [1, 3], {})["weights"] == [0.25, 0.75]


@pytest.mark.parametrize("bad,n", [([1.0, -0.1], 2), ([0.0, 0.0], 2), ([1.0], 2), ([1.0, 2.0, 3.0], 2), ([float("nan"), 1.0], 2),
                                   ([float("inf"), 1.0], 2)])
def test_bad_weights_raise_value_error(bad, n):
    with pytest.raises(ValueError):
        search.ensemble_weights(bad, n)
    with pytest.raises(ValueError):
        search.ensemble_plan("product", n, bad, {})


def test_select_takes_no_weights():
    with pytest.raises(ValueError, match="select"):
        search.ensemble_plan("select", 2, [1, 1], {})


def _t5_stub():
    return SimpleNamespace(lm=SimpleNamespace(cfg=SimpleNamespace(eos_token_id=1)))


def _causal_stub(weight_format="native"):
    return SimpleNamespace(gpt=SimpleNamespace(weight_format=weight_format, cfg=SimpleNamespace(eos_token_id=1, pad_token_id=0)))


@pytest.mark.parametrize("kw,name", [
    (dict(num_beams=3), "num_beams"),
    (dict(num_return_sequences=2), "num_return_sequences"),
    (dict(decoder_input_ids=torch.zeros(2, 1, dtype=torch.long)), "decoder_input_ids"),
    (dict(pass_examples_through_encoder_one_at_a_time=True), "pass_examples_through_encoder_one_at_a_time"),
])
def test_entry_points_reject_before_anything_runs(kw, name):
    """The stubs hold no weights and no device: a call that got past the argument rules would fail on them with another exception."""
    tok = torch.zeros(2, 3, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match=name):
        VCT0Model.generate_ensemble(_t5_stub(), prefix=None, question_tokens=tok, **kw)
    with pytest.raises(NotImplementedError, match=name):
        ClipCaptionModel._generate_ensemble(_causal_stub(), None, 2, 3, "product", None, **kw)


def test_entry_points_reject_fp8_weights_nine_members_and_bad_weights():
    with pytest.raises(NotImplementedError, match="lm_weight_format"):
        ClipCaptionModel._generate_ensemble(_causal_stub("fp8"), None, 2, 3, "mixture", None)
    with pytest.raises(NotImplementedError, match="n=9"):
        VCT0Model.generate_ensemble(_t5_stub(), prefix=None, question_tokens=torch.zeros(2, 9, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="n=9"):
        ClipCaptionModel._generate_ensemble(_causal_stub(), None, 2, 9, "product", None)
    with pytest.raises(ValueError):
        VCT0Model.generate_ensemble(_t5_stub(), prefix=None, question_tokens=torch.zeros(2, 3, 4, dtype=torch.long), ensemble_weights=[1, -1, 1])
    with pytest.raises(ValueError):
        ClipCaptionModel._generate_ensemble(_causal_stub(), None, 2, 3, "product", [0, 0, 0])
    with pytest.raises(ValueError, match=r"\[B, n, T\]"):
        VCT0Model.generate_ensemble(_t5_stub(), prefix=None, question_tokens=torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="unsupported generation arguments"):
        VCT0Model.generate_ensemble(_t5_stub(), prefix=None, question_tokens=torch.zeros(2, 3, 4, dtype=torch.long), penalty_alpha=0.5)


def test_select_members_keeps_the_first_best_member_cut_where_its_own_batch_stops():
    """B = 2 questions x n = 2 members, T5 layout (a start column, eos = 1, pad = 0).  Member 0's rows end after 2 and 3 tokens, member 1's
    after 4 and 1: a generation of member 0 alone would have 1 + 3 columns, of member 1 alone 1 + 4."""
    seq = torch.tensor([[0, 5, 1, 0, 0],        # q0 m0
                        [0, 6, 7, 8, 1],        # q0 m1
                        [0, 9, 2, 1, 0],        # q1 m0
                        [0, 1, 0, 0, 0]])       # q1 m1
    logp = torch.tensor([[-1.0, -9.0, -9.0, -9.0],          # -1 (eos, pads ignored)
                         [-0.2, -0.2, -0.2, -9.0],          # -0.6: the best of q0
                         [-0.5, -9.0, -9.0, -9.0],          # -0.5 (2 and eos ignored)
                         [-9.0, -9.0, -9.0, -9.0]])         # 0: nothing scored - the best of q1
    out = search.select_members(seq, logp, 2, 2, 1, 0, 1, (0, 1, 2))
    assert out.tolist() == [[0, 6, 7, 8, 1], [0, 1, 0, 0, 0]]
    tie = search.select_members(seq[[0, 0, 2, 2]], logp[[0, 0, 2, 2]], 2, 2, 1, 0, 1, (0, 1, 2))
    assert tie.tolist() == [[0, 5, 1, 0], [0, 9, 2, 1]]              # equal scores: member 0, cut at its batch's 3 tokens
    no_eos = search.select_members(seq, logp, 2, 2, 1, 0, None, (0, 1, 2))
    assert no_eos.shape == (2, 5)


def _combine(lib, **over):
    """``eavqa_ensemble_combine`` on a small valid problem (16 / 4096 / 8192 stand for aligned pointers) with the named arguments replaced."""
    a = dict(B=2, n=3, V=10, logits=4096, ld=12, mode=0, weights=None, out=8192, ld_out=12, stats=16, member_lse=None, stream=None)
    assert not set(over) - set(a), over
    a.update(over)
    return lib.eavqa_ensemble_combine(*[a[k] for k in ("B", "n", "V", "logits", "ld", "mode", "weights", "out", "ld_out", "stats", "member_lse",
                                                       "stream")])


@pytest.mark.parametrize("fault", [dict(n=9), dict(n=0), dict(out=4096), dict(ld=9), dict(ld_out=9), dict(logits=None), dict(out=None),
                                   dict(stats=None), dict(mode=2), dict(B=0), dict(V=0)])
def test_combine_rejects_bad_arguments_before_any_launch(fault):
    """No device exists here: a call that got as far as a launch would not return EAVQA_E_ARG."""
    from eavqa_amd import _lib, build
    build.build()
    assert _combine(_lib.load(), **fault) == -1
