"""CPU: the host plan of the logits processors (``models/logits_process.py``) rejects what it must and names the argument, the two
generate paths accept the five names, ``eavqa_logits_process`` / ``eavqa_beam_step_logprobs`` validate before any launch, and the
reference fixture tests/golden/vct0_logits.npz holds what its generator promises."""
import dataclasses

import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


def plan(**kw):
    from eavqa_amd.models.logits_process import processing_plan
    return processing_plan(dict(dict(eos_token_id=1, max_length=10), **kw))


# ------------------------------------------------------------------------------------------------ processing_plan
def test_nothing_active_is_no_plan():
    assert plan() is None
    assert plan(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, bad_words_ids=None) is None
    assert plan(repetition_penalty=None, no_repeat_ngram_size=None, min_length=None, min_new_tokens=None) is None
    assert plan(min_new_tokens=0) is None
    assert plan(bad_words_ids=[[1]]) is None                       # [eos] is dropped, as HF does: nothing is left


def test_plan_fields_and_defaults():
    from eavqa_amd.models.logits_process import LogitsPlan
    p = plan(repetition_penalty=1.2)
    assert p == LogitsPlan(repetition_penalty=1.2, eos_token_id=1) and dataclasses.is_dataclass(p)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.repetition_penalty = 2.0
    assert plan(repetition_penalty=0.5).repetition_penalty == 0.5   # values < 1 are legal
    assert plan(repetition_penalty=2).repetition_penalty == 2.0
    assert plan(no_repeat_ngram_size=3).no_repeat_ngram_size == 3
    assert plan(min_length=10).min_length == 10 and plan(min_new_tokens=4).min_new_tokens == 4
    p = plan(bad_words_ids=[[7], [1], [3, 4], [7], (5, 6, 7)])
    assert p.bad_words == ((7,), (3, 4), (5, 6, 7))                 # [eos] dropped, a repeated word once
    assert plan(bad_words_ids=[[1, 2]], eos_token_id=None).eos_token_id is None          # bad words need no eos


def test_suppress_eos_is_hfs_two_length_rules():
    p = plan(min_length=4)
    assert [p.suppress_eos(t, 1) for t in (1, 3, 4, 5)] == [True, True, False, False]
    p = plan(min_new_tokens=3)
    assert [p.suppress_eos(t, 1) for t in (1, 3, 4)] == [True, True, False]
    assert [p.suppress_eos(t, 0) for t in (0, 2, 3)] == [True, True, False]       # the causal path: HF's input_ids start empty
    assert not plan(no_repeat_ngram_size=2).suppress_eos(0, 1)


REJECTED = [
    ("repetition_penalty", 0.0, ValueError), ("repetition_penalty", -1.0, ValueError), ("repetition_penalty", float("inf"), ValueError),
    ("repetition_penalty", float("nan"), ValueError), ("repetition_penalty", "1.2", ValueError), ("repetition_penalty", True, ValueError),
    ("no_repeat_ngram_size", -1, ValueError), ("no_repeat_ngram_size", 2.0, ValueError),
    ("min_length", -1, ValueError), ("min_length", 11, ValueError), ("min_length", 1.5, ValueError),
    ("min_new_tokens", -2, ValueError), ("min_new_tokens", 11, ValueError),
    ("bad_words_ids", [], ValueError), ("bad_words_ids", [[]], ValueError), ("bad_words_ids", [3], ValueError),
    ("bad_words_ids", [[-1]], ValueError), ("bad_words_ids", [[1.0]], ValueError), ("bad_words_ids", "ab", ValueError),
    ("bad_words_ids", [[2]] * 1025, NotImplementedError), ("bad_words_ids", [list(range(2, 19))], NotImplementedError),
]


@pytest.mark.parametrize("name,value,exc", REJECTED, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(REJECTED)])
def test_every_rejection_names_its_argument(name, value, exc):
    with pytest.raises(exc, match=name):
        plan(**{name: value})


def test_length_rules_need_an_eos_and_exclude_each_other():
    with pytest.raises(ValueError, match="min_length.*eos_token_id"):
        plan(min_length=3, eos_token_id=None)
    with pytest.raises(ValueError, match="min_new_tokens.*eos_token_id"):
        plan(min_new_tokens=3, eos_token_id=None)
    with pytest.raises(ValueError, match="min_length together with min_new_tokens"):
        plan(min_length=3, min_new_tokens=2)
    assert plan(bad_words_ids=[[2]] * 1024) is not None and plan(bad_words_ids=[list(range(2, 18))]) is not None     # the limits themselves


def test_numpy_integers_and_floats_are_taken_as_hf_takes_them():
    """Fixture-driven callers pass ``np.int64`` ids and sizes; a numpy bool or float where an integer belongs is still rejected."""
    from eavqa_amd.models.logits_process import LogitsPlan
    p = plan(repetition_penalty=np.float32(1.5), no_repeat_ngram_size=np.int64(2), min_length=np.int32(4),
             bad_words_ids=[[np.int64(7)], list(np.array([3, 4])), [np.int64(1)]], eos_token_id=np.int64(1))
    assert p == LogitsPlan(1.5, 2, 4, 0, ((7,), (3, 4)), 1)
    assert all(type(t) is int for w in p.bad_words for t in w) and type(p.no_repeat_ngram_size) is int and type(p.eos_token_id) is int
    assert plan(min_new_tokens=np.int64(3)).min_new_tokens == 3
    for name, value in (("no_repeat_ngram_size", np.float64(2.0)), ("min_length", np.bool_(True)), ("bad_words_ids", [[np.float32(3.0)]])):
        with pytest.raises(ValueError, match=name):
            plan(**{name: value})


def test_a_history_longer_than_the_kernel_holds_is_rejected_once_on_the_host():
    """``eavqa_logits_process`` stages at most 2048 history ids, and a history never passes ``max_length``: the plan says so before the
    loop starts, not the kernel in the middle of it.  Without a rule there is no plan and no limit."""
    from eavqa_amd.models.logits_process import MAX_HISTORY
    assert MAX_HISTORY == 2048 and plan(no_repeat_ngram_size=2, max_length=MAX_HISTORY) is not None
    with pytest.raises(NotImplementedError, match="max_length"):
        plan(no_repeat_ngram_size=2, max_length=MAX_HISTORY + 1)
    assert plan(max_length=MAX_HISTORY + 1) is None and plan(repetition_penalty=1.0, max_length=10 ** 6) is None
    assert plan(repetition_penalty=1.2, max_length=None) is not None


def test_bad_word_ids_beyond_the_vocabulary_are_rejected_at_upload():
    with pytest.raises(ValueError, match="bad_words_ids"):
        plan(bad_words_ids=[[5, 99]]).upload(50, "cpu")
    d = plan(bad_words_ids=[[5, 49], [7]]).upload(50, "cpu")
    assert d.bad_words.tolist() == [[5, 49], [7, 0]] and d.bad_lens.tolist() == [2, 1] and (d.n_bad, d.bad_width) == (2, 2)


# ------------------------------------------------------------------------------------------------ the two generate paths
def test_generation_plan_accepts_the_names_and_is_unchanged_without_them():
    from eavqa_amd.models.logits_process import LogitsPlan
    from eavqa_amd.models.vct0 import generation_plan
    base = dict(num_beams=1, num_return_sequences=1, length_penalty=1.0, early_stopping=False, eos_token_id=None)
    assert generation_plan({}) == base
    assert generation_plan(dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=None)) == base       # nothing active: no key
    got = generation_plan(dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=3, bad_words_ids=[[4, 5]]), max_length=10,
                          config_eos_token_id=1)
    assert got == dict(base, logits=LogitsPlan(1.2, 2, 0, 3, ((4, 5),), 1))
    # the call's eos id wins over the config's; beams, sampling and the decoder prompt take the plan too
    assert generation_plan(dict(min_length=3, eos_token_id=7, num_beams=3), config_eos_token_id=1)["logits"].eos_token_id == 7
    assert generation_plan(dict(no_repeat_ngram_size=1, do_sample=True, num_return_sequences=4))["logits"].no_repeat_ngram_size == 1
    assert "logits" in generation_plan(dict(repetition_penalty=1.3), decoder_input_ids=object())
    with pytest.raises(ValueError, match="min_length"):
        generation_plan(dict(min_length=11), max_length=10, config_eos_token_id=1)
    for name in ("encoder_repetition_penalty", "encoder_no_repeat_ngram_size", "sequence_bias", "suppress_tokens", "forced_eos_token_id"):
        with pytest.raises(NotImplementedError, match=name):
            generation_plan({name: 1})
    with pytest.raises(NotImplementedError, match="eos_token_id"):
        generation_plan(dict(eos_token_id=[1, 2], min_length=2))


def test_causal_entry_takes_the_names_out_before_the_sampler_sees_them():
    from eavqa_amd.models.logits_process import split_logits_kwargs
    from eavqa_amd.models.sampling import causal_sampler
    rest, procs = split_logits_kwargs(dict(do_sample=True, seed=3, repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=1, min_new_tokens=None,
                                           bad_words_ids=[[3]]))
    assert rest == dict(do_sample=True, seed=3) and sorted(procs) == sorted(["repetition_penalty", "no_repeat_ngram_size", "min_length",
                                                                             "min_new_tokens", "bad_words_ids"])
    assert causal_sampler(object.__new__(type("M", (), {})), rest).seed == 3
    with pytest.raises(TypeError, match="num_beams"):
        causal_sampler(None, split_logits_kwargs(dict(num_beams=2, repetition_penalty=1.3))[0])


# ------------------------------------------------------------------------------------------------ the entry points, before any launch
P = 4096      # a non-null, 16-byte aligned value standing in for a device pointer: every call below must return before it is used


def _process(lib, **over):
    a = dict(R=2, V=32, scores=P, ld=32, to_logprobs=0, history=P, ld_history=8, cur_len=3, rp=1.2, ngram=2, eos=1, suppress=0, words=None,
             lens=None, n_bad=0, width=0)
    assert not set(over) - set(a)
    a.update(over)
    return lib.eavqa_logits_process(a["R"], a["V"], a["scores"], a["ld"], a["to_logprobs"], a["history"], a["ld_history"], a["cur_len"], a["rp"],
                                    a["ngram"], a["eos"], a["suppress"], a["words"], a["lens"], a["n_bad"], a["width"], None)


def test_logits_process_rejects_bad_arguments_before_any_launch(lib):
    assert _process(lib, scores=None) == -1 and _process(lib, history=None) == -1 and _process(lib, R=0) == -1 and _process(lib, V=0) == -1
    assert _process(lib, cur_len=-1) == -1 and _process(lib, to_logprobs=2) == -1 and _process(lib, suppress=2) == -1
    assert _process(lib, rp=0.0) == -1 and _process(lib, rp=-1.0) == -1 and _process(lib, rp=float("nan")) == -1 and _process(lib, rp=float("inf")) == -1
    assert _process(lib, ngram=-1) == -1 and _process(lib, n_bad=-1) == -1
    assert _process(lib, n_bad=1, width=1) == -1 and _process(lib, n_bad=1, words=P, width=1) == -1          # a table needs both arrays
    assert _process(lib, n_bad=1, words=P, lens=P, width=0) == -1
    assert _process(lib, suppress=1, eos=-1) == -1
    assert _process(lib, V=33) == -3 and _process(lib, cur_len=9) == -3                                        # V > ld, cur_len > ld_history
    assert _process(lib, cur_len=2049, ld_history=4096) == -3
    assert _process(lib, n_bad=1025, words=P, lens=P, width=1) == -3 and _process(lib, n_bad=1, words=P, lens=P, width=17) == -3


def test_beam_step_logprobs_rejects_what_beam_step_rejects(lib):
    def step(B=2, k=2, V=32, ld=32, cur_len=1, max_length=8, ptrs=None, ws=P, ws_bytes=1 << 20):
        ptrs = [P] * 11 if ptrs is None else ptrs
        return lib.eavqa_beam_step_logprobs(B, k, V, ptrs[0], ld, cur_len, max_length, 1, 1.0, 1.0, 0, *ptrs[1:], ws, ws_bytes, None)

    for i in range(11):
        assert step(ptrs=[None if j == i else P for j in range(11)]) == -1
    assert step(ws=None) == -1 and step(k=9) == -3 and step(k=0) == -3 and step(V=33) == -3 and step(k=8, V=15, ld=16) == -3
    assert step(cur_len=8) == -1 and step(cur_len=0) == -1 and step(B=0) == -1
    assert step(ws_bytes=lib.eavqa_beam_step_workspace_bytes(2, 2) - 1) == -1


# ------------------------------------------------------------------------------------------------ the fixture
MARGIN = 1e-3


@pytest.mark.parametrize("tag", ["t0", "t5v10"])
def test_fixture_conditions_are_recomputed_from_the_committed_arrays(tag):
    z = load_golden("vct0_logits.npz")
    cases = z["cases"].tolist()
    assert cases == ["g_rp", "g_ng2", "g_ng1", "g_minlen", "g_bad", "g_all", "b_rp_ng", "b_minlen", "p_ng2"]
    assert z["paths"].tolist() == ["fs"] * 8 + ["prefix"]
    for name in cases:
        f = lambda field: z[f"{tag}.{name}.{field}"]
        k, max_length, eos, ngram, min_length, min_new = [int(v) for v in f("params")]
        seq, plain = f("sequences"), f("plain")
        assert float(f("min_gap")) >= MARGIN, name
        assert seq.shape != plain.shape or not np.array_equal(seq, plain), name                   # the processors changed the output
        assert seq.shape[0] == 3 * k and seq.shape[1] <= max_length == (8 if k > 1 else 10)
        assert (name[0] == "b") == (k == 3) and (f"{tag}.{name}.sequences_scores" in z) == (k > 1)
        end = 1 if eos < 0 else eos
        for row in seq:
            body = row[1:].tolist()
            stop = body.index(end) if end in body else len(body)
            toks = body[:stop]                                                                    # what the row generated before its eos
            if ngram == 1:
                assert len(set(toks)) == len(toks), name
            if ngram == 2:
                grams = list(zip(row[:stop + 1].tolist(), row[1:stop + 1].tolist()))
                assert len(set(grams)) == len(grams), name
            if min_length:
                assert 1 + stop >= min_length, name               # eos is first allowed at a history of min_length ids
            if min_new:
                assert stop >= min_new, name
            words = [[int(t) for t in w if t >= 0] for w in f("bad_words")]
            full = row[:stop + 1].tolist()
            for w in words:
                assert not any(full[i:i + len(w)] == w for i in range(len(full))), (name, w)
        if name == "g_bad":
            assert sorted(len(w) for w in words) == [1, 2] and any((plain == words[0][0]).any(axis=1))
        if min_length or min_new:
            assert eos > 1 and (plain[:, 1:] == eos).any()        # an eos the model really emits without the rule
    assert float(z[f"{tag}.g_rp.repetition_penalty"]) == 1.5 and float(z[f"{tag}.g_all.repetition_penalty"]) == 1.3
    assert float(z[f"{tag}.b_rp_ng.repetition_penalty"]) == 1.3 and float(z[f"{tag}.g_ng2.repetition_penalty"]) == 1.0
