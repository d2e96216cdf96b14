"""GPU: ensemble decoding end to end - ``VCT0Model.generate_ensemble`` on both tiny T5 fixtures and ``ClipCaptionModel.generate_ensemble``
/ ``generate_ensemble_fewshot`` on both tiny causal models (fp32, the committed weights loaded as tests/_search_modes.py does; B = 3
questions x n = 3 members, ``max_length`` = 6; inputs and CPU replays in tests/_ensemble_cases.py).  Identical members and one-hot
weights must reproduce the plain call; distinct members are replayed through the CPU oracle and tests/_ensemble_ref.py; "select" must
return what ``FewShotVQAExecutor.generate_from_ensembles`` (``utils.ensembling.generate_from_ensembles`` on the causal path) returns;
rules and sampling are replayed from the combined scores with the references of their own kernels."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _constrained_ref as cref
import _ensemble_cases as ec
import _ensemble_ref as eref
import _logits_ref as lref
import _sampling_ref as R
import _search_modes as sm

DEV = "cuda"
B, N, ML = ec.B, ec.N, ec.MAX_LENGTH
MODES = ("product", "mixture")
NEG_INF = float("-inf")
RETURN = dict(output_scores=True, return_dict_in_generate=True)


@pytest.fixture
def combined(monkeypatch):
    """Every ``ops.ensemble_combine`` result of the calls that follow, copied to the host as float32 [B, V] in launch order - the combined
    scores BEFORE the rules and the pick (the loop may run up to three steps past the stop: only the first ones belong to the ids)."""
    from eavqa_amd import ops
    seen, real = [], ops.ensemble_combine

    def spy(logits, V, *a, **k):
        out = real(logits, V, *a, **k)
        seen.append(out[:, :V].clone())
        return out
    monkeypatch.setattr(ops, "ensemble_combine", spy)
    return lambda: [x.cpu() for x in seen]


def _causal(arch):
    """(model, plain call [B, N, ...], few-shot call [B, N, ...], eos, V, the common keywords)."""
    model, plain, few, eos, V = sm.causal_model(arch)
    p, f = ec.causal_members(plain, few, V)
    return model, p, f, eos, V, dict(max_length=ML, pad_token_id=sm.CAUSAL_PAD, eos_token_id=eos)


def _causal_entries(arch):
    """[(ensemble entry point, the plain entry point, the [B, N, ...] call)] of one causal model."""
    model, p, f, eos, V, kw = _causal(arch)
    return [(model.generate_ensemble, model.generate, p), (model.generate_ensemble_fewshot, model.generate_fewshot, f)], eos, V, kw


# ------------------------------------------------------------------------------------------------ 1. identical members
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", sm.T5_TAGS)
def test_t5_identical_members_give_the_plain_generation(tag, mode):
    model = sm.t5_model(tag)[0]
    call = ec.t5_member_call(tag, 0)
    plain = model.generate(max_length=ML, **RETURN, **call)
    got = model.generate_ensemble(ensemble=mode, max_length=ML, **RETURN, **ec.repeated(call))
    assert torch.equal(got.sequences, plain.sequences)
    want = torch.log_softmax(torch.stack(list(plain.scores)), dim=-1)
    have = torch.stack(list(got.scores))
    assert have.shape == want.shape and (have - want).abs().max().item() <= 1e-3          # the tolerance of tests/test_t5_gpu.py:251
    assert torch.equal(model.generate_ensemble(ensemble=mode, max_length=ML, **ec.repeated(call)), plain.sequences)      # a tensor, as generate
    text = model.generate(max_length=ML, no_prefix=True, bad_words_ids=[[0]], **call)                                    # the text-only input form
    assert torch.equal(model.generate_ensemble(ensemble=mode, max_length=ML, no_prefix=True, bad_words_ids=[[0]], **ec.repeated(call)), text)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("arch", list(sm.CAUSAL))
def test_causal_identical_members_give_the_plain_generation(arch, mode):
    entries, eos, V, kw = _causal_entries(arch)
    for ensemble, plain, call in entries:
        one = ec.member_of(call, 0)
        want, want_lp = plain(output_scores=True, **one, **kw)
        got, lp = ensemble(ensemble=mode, output_scores=True, **ec.repeated(one), **kw)
        assert got == want
        assert lp.shape == want_lp.shape and (lp - want_lp).abs().max().item() <= 1e-3
        assert ensemble(ensemble=mode, **ec.repeated(one), **kw) == want


# ------------------------------------------------------------------------------------------------ 2. one-hot weights
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", sm.T5_TAGS)
def test_t5_one_hot_weights_give_that_members_generation(tag, mode):
    model = sm.t5_model(tag)[0]
    for hot in range(N):
        w = [0.0] * N
        w[hot] = 3.0
        got = model.generate_ensemble(ensemble=mode, ensemble_weights=w, max_length=ML, **ec.t5_members(tag))
        assert torch.equal(got, model.generate(max_length=ML, **ec.t5_member_call(tag, hot))), hot


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("arch", list(sm.CAUSAL))
def test_causal_one_hot_weights_give_that_members_generation(arch, mode):
    entries, eos, V, kw = _causal_entries(arch)
    for ensemble, plain, call in entries:
        for hot in range(N):
            w = [0.0] * N
            w[hot] = 1.0
            assert ensemble(ensemble=mode, ensemble_weights=w, **call, **kw) == plain(**ec.member_of(call, hot), **kw), hot


# ------------------------------------------------------------------------------------------------ 3. distinct members against the oracle
@pytest.mark.parametrize("banned", [(), (0,)], ids=["plain", "no_pad"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", sm.T5_TAGS)
def test_t5_distinct_members_match_the_oracle(tag, mode, banned):
    """The returned ids replayed teacher-forced through oracle/ref_cpu.py member by member, the members combined by
    tests/_ensemble_ref.py: scores within 1e-3, ids = the oracle's argmax at every step.  A step could be left out of the id check if
    the oracle's top-two margin there were below 2e-3; tests/_ensemble_cases.py chose its seed on the CPU so that none is.  ``no_pad``:
    the tiny models prefer id 0 (the pad) at every step, so the same check also runs with ``bad_words_ids=[[0]]`` - other ids, and
    the rule acts on the combined row."""
    model = sm.t5_model(tag)[0]
    rules = dict(bad_words_ids=[[t] for t in banned]) if banned else {}
    got = model.generate_ensemble(ensemble=mode, max_length=ML, **RETURN, **rules, **ec.t5_members(tag))
    ids, have = got.sequences, torch.stack(list(got.scores)).double()
    assert ids.shape == (B, ML) and have.shape[0] == ML - 1
    want = ec.ban(ec.t5_oracle_scores(tag, ids, mode), banned)
    assert torch.equal(torch.isinf(have), torch.isinf(want))
    fin = ~torch.isinf(want)
    err = (have[fin] - want[fin]).abs().max().item()
    margin = ec.margins(want)
    print(f"[{tag} {mode} banned={banned}] max |score - oracle| {err:.2e}, smallest oracle top-two margin {margin.min().item():.3e}")
    assert err <= 1e-3
    left_out = margin < 2e-3
    assert not left_out.any()
    assert torch.equal(ids[:, 1:].t()[~left_out], want.argmax(-1)[~left_out])
    if banned:
        assert not (ids[:, 1:] == 0).any()
    assert torch.equal(ids, ec.oracle_greedy(tag, mode, banned=banned)[0])


# ------------------------------------------------------------------------------------------------ 4. select
def _few_shot_executor(tag, **additional):
    from eavqa_amd.trainers.vct0_executor import FewShotVQAExecutor
    from eavqa_amd.utils import config_system as cs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model, _, _, _, V = sm.t5_model(tag)
    few = cs.load_config(os.path.join(root, "configs", "vqa2", "few_shot_vqa_t0_3b.jsonnet"), mode="test",
                         opts=[f"data_loader.additional.special_token_id={V - 1}", f"data_loader.additional.max_target_length={ML}"])
    for k, v in additional.items():
        setattr(few.data_loader.additional, k, v)
    return FewShotVQAExecutor(few, model=model, dtype=torch.float32, device=DEV), few


def _same_up_to_the_pad_tail(got_row, want_row, pad):
    got_row, want_row = [int(t) for t in got_row], [int(t) for t in want_row]
    return got_row[:len(want_row)] == want_row and all(t == pad for t in got_row[len(want_row):])


@pytest.mark.parametrize("eos", [None, "emitted"])
@pytest.mark.parametrize("tag", sm.T5_TAGS)
def test_t5_select_is_generate_from_ensembles(tag, eos):
    """``eos="emitted"``: the tiny models never emit T5's eos, so it is moved onto a token some member does emit (the first one that is
    not the pad id, else the pad id itself) - rows then end at different steps, and the members' own generations differ in length."""
    fx, _ = _few_shot_executor(tag)
    m = ec.t5_members(tag)
    cfg = fx.model.lm.cfg
    old = cfg.eos_token_id
    try:
        if eos is not None:
            emitted = [t for i in range(N) for t in fx.model.generate(max_length=ML, **ec.t5_member_call(tag, i))[:, 1:].reshape(-1).tolist()]
            cfg.eos_token_id = next((t for t in emitted if t != cfg.pad_token_id), cfg.pad_token_id)
        want = fx.generate_from_ensembles(m["question_tokens"].to(DEV), m["question_mask"].to(DEV), m["prefix"].to(DEV), N, ML,
                                          sentinel=m["special_token_id"])
        got = fx.model.generate_ensemble(ensemble="select", max_length=ML, **m)
    finally:
        cfg.eos_token_id = old
    assert got.shape[0] == B and got.shape[1] == max(len(w) for w in want)
    for b in range(B):
        assert _same_up_to_the_pad_tail(got[b], want[b], cfg.pad_token_id), (b, got[b], want[b])


@pytest.mark.parametrize("arch", list(sm.CAUSAL))
def test_causal_select_is_generate_from_ensembles(arch):
    from eavqa_amd.utils import ensembling
    entries, eos, V, kw = _causal_entries(arch)
    for ensemble, plain, call in entries:
        want = ensembling.generate_from_ensembles(lambda i: plain(output_scores=True, **ec.member_of(call, i), **kw), N)
        got = ensemble(ensemble="select", **call, **kw)
        assert len(got) == B
        for b in range(B):
            assert _same_up_to_the_pad_tail(got[b], want[b], sm.CAUSAL_PAD), (b, got[b], want[b])


# ------------------------------------------------------------------------------------------------ 5. rules
def _replay_rules(raw_steps, ids, first, eos, pad, sequences, penalty):
    """The rules' references on the combined scores of every step: ``(processed [steps, B, V], ids the argmax gives)``; a row that has
    produced eos emits pad."""
    processed, picks = [], []
    done = torch.zeros(ids.shape[0], dtype=torch.bool)
    for j in range(ids.shape[1] - first):
        t = first + j
        s = lref.process(raw_steps[j], ids[:, :t], repetition_penalty=penalty)
        s = cref.mask(s, ids, first, t, eos, sequences=sequences)
        processed.append(s)
        pick = torch.where(done, torch.full_like(ids[:, 0], pad), s.argmax(-1))
        picks.append(pick)
        done = done | (pick == eos)
    return torch.stack(processed), torch.stack(picks, dim=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", sm.T5_TAGS)
def test_t5_rules_run_on_the_combined_scores(tag, mode, combined):
    model, _, _, eos, V = sm.t5_model(tag)
    answers = sm.answer_set(V, 3)
    got = model.generate_ensemble(ensemble=mode, max_length=ML, allowed_sequences=answers, **sm.RULES, **RETURN, **ec.t5_members(tag))
    ids, have = got.sequences, torch.stack(list(got.scores))
    for row in ids.tolist():
        body, full = cref.cut(row, eos, 1), eos in row[1:]
        assert any((m == body) if full else (m[:len(body)] == body and len(body) == ML - 1) for m in answers), row
    raw = combined()[:ids.shape[1] - 1]
    want, picks = _replay_rules(raw, ids, 1, eos, model.lm.cfg.pad_token_id, answers, sm.RULES["repetition_penalty"])
    assert have.shape == want.shape and torch.equal(have.view(torch.int32), want.view(torch.int32))
    assert torch.equal(ids[:, 1:], picks)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("arch", list(sm.CAUSAL))
def test_causal_rules_run_on_the_combined_scores(arch, mode, combined):
    entries, eos, V, kw = _causal_entries(arch)
    answers = sm.answer_set(V, 3)
    done = 0
    for ensemble, plain, call in entries:
        ids = torch.tensor(ensemble(ensemble=mode, allowed_sequences=answers, **sm.RULES, **call, **kw))
        for row in ids.tolist():
            body, full = cref.cut(row, eos, 0), eos in row
            assert any((m == body) if full else (m[:len(body)] == body and len(body) == ML) for m in answers), row
        raw = combined()[done:]
        done += len(raw)
        _, picks = _replay_rules(raw[:ids.shape[1]], ids, 0, eos, sm.CAUSAL_PAD, answers, sm.RULES["repetition_penalty"])
        assert torch.equal(ids, picks)


# ------------------------------------------------------------------------------------------------ 6. sampling
def _replay_draws(ids, processed, first, seed, eos):
    """tests/test_sample_gpu.py's check: every drawn id is the inverse-CDF pick of its own processed scores under the reference Philox
    (uniform of (seed, decoder position, row)); a draw within 1e-5 of a CDF boundary is left out, and few may be."""
    pairs = skipped = 0
    for r in range(ids.shape[0]):
        for j, sc in enumerate(processed):
            t = first + j
            tok = int(ids[r, t])
            u = R.philox_uniform(seed, t, r)
            pairs += 1
            if R.cdf_margin(sc[r], u) < 1e-5:
                skipped += 1
            else:
                assert tok == R.inverse_cdf(sc[r], u), (r, t)
            assert math.isfinite(float(sc[r, tok]))
            if tok == eos:
                break
    assert pairs >= ids.shape[0] and skipped <= 0.02 * pairs, (skipped, pairs)


SAMPLING = dict(do_sample=True, temperature=1.3, top_k=0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", sm.T5_TAGS)
def test_t5_sampling_replays_from_its_scores_and_the_reference_philox(tag, mode):
    model, _, _, eos, V = sm.t5_model(tag)
    kw = dict(ensemble=mode, max_length=ML, **SAMPLING, **RETURN, **ec.t5_members(tag))
    seed = 424242
    out = model.generate_ensemble(seed=seed, **kw)
    ids, scores = out.sequences, out.scores
    assert ids.shape[0] == B and len(scores) == ids.shape[1] - 1 and tuple(scores[0].shape) == (B, V)
    _replay_draws(ids, scores, 1, seed, eos)
    again, other = model.generate_ensemble(seed=seed, **kw), model.generate_ensemble(seed=seed + 1, **kw)
    assert torch.equal(again.sequences, ids)
    assert other.sequences.shape != ids.shape or not torch.equal(other.sequences, ids)
    assert len(set(ids[:, 1:].reshape(-1).tolist())) > 1                    # a free run, not the greedy ids


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("arch", list(sm.CAUSAL))
def test_causal_sampling_replays_from_the_combined_scores(arch, mode, combined):
    """The causal path returns no [B, V] scores: the processed scores of a step are tests/_sampling_ref.py's warp of the combined row."""
    model, p, f, eos, V, kw = _causal(arch)
    seed = 99
    ids = torch.tensor(model.generate_ensemble(ensemble=mode, seed=seed, **SAMPLING, **p, **kw))
    raw = combined()[:ids.shape[1]]
    processed = [R.warp(x, SAMPLING["temperature"], 0, 1.0) for x in raw]
    _replay_draws(ids, processed, 0, seed, eos)
    assert model.generate_ensemble(ensemble=mode, seed=seed, **SAMPLING, **p, **kw) == ids.tolist()
    assert model.generate_ensemble(ensemble=mode, seed=seed + 1, **SAMPLING, **p, **kw) != ids.tolist()


# ------------------------------------------------------------------------------------------------ 7. use_cache=False
@pytest.mark.parametrize("mode", MODES + ("select",))
@pytest.mark.parametrize("tag", sm.T5_TAGS)
def test_t5_without_a_cache_gives_the_cached_ids(tag, mode):
    model = sm.t5_model(tag)[0]
    kw = dict(ensemble=mode, max_length=ML, bad_words_ids=[[0]], **ec.t5_members(tag))
    cached = model.generate_ensemble(use_cache=True, **kw)
    assert torch.equal(model.generate_ensemble(use_cache=False, **kw), cached)
    model.lm.native_step = False                                            # the cached steps issued from Python
    try:
        assert torch.equal(model.generate_ensemble(use_cache=True, **kw), cached)
    finally:
        model.lm.native_step = True


@pytest.mark.parametrize("mode", MODES + ("select",))
@pytest.mark.parametrize("arch", list(sm.CAUSAL))
def test_causal_without_a_cache_gives_the_cached_ids(arch, mode):
    entries, eos, V, kw = _causal_entries(arch)
    for ensemble, plain, call in entries:
        assert ensemble(ensemble=mode, use_cache=False, **call, **kw) == ensemble(ensemble=mode, use_cache=True, **call, **kw)


# ------------------------------------------------------------------------------------------------ 8. the executor
def _candidate_tensor(members, width):
    out = torch.full((len(members), width), -100, dtype=torch.int64)
    for j, m in enumerate(members):
        out[j, :len(m)] = torch.tensor(m)
    return out


@pytest.mark.parametrize("decoding", MODES + ("select",))
def test_executor_decodes_ensembles_when_the_config_asks_for_it(decoding):
    tag = "t0"
    m = ec.t5_members(tag)
    V = m["special_token_id"] + 1
    batch = {"generative_input_ids": m["question_tokens"].reshape(B * N, -1), "generative_attention_mask": m["question_mask"].reshape(B * N, -1),
             "clip_embeddings": m["prefix"]}
    fx, few = _few_shot_executor(tag, num_permutations_of_in_context_examples=N, ensemble_decoding=decoding)
    step = fx._generative_step(batch, 0)
    assert len(step["predictions"]) == B
    assert torch.equal(step["outputs"], fx.model.generate_ensemble(ensemble=decoding, max_length=ML, **m))
    drawn = fx._generative_step(batch, 0, do_sample=True, seed=5, top_k=0, temperature=1.3)
    assert len(drawn["predictions"]) == B and torch.equal(drawn["outputs"], fx._generative_step(batch, 0, do_sample=True, seed=5, top_k=0,
                                                                                                 temperature=1.3)["outputs"])
    answers = sm.answer_set(V, 3)
    out = fx.answer_from_set(batch, _candidate_tensor(answers, 5))
    assert len(out["predictions"]) == B
    for row in out["outputs"].tolist():
        body, full = cref.cut(row, 1, 1), 1 in row[1:]
        assert any((a == body) if full else (a[:len(body)] == body and len(body) == ML - 1) for a in answers), row
    # without the key: today's behaviour, both refusals included
    del few.data_loader.additional["ensemble_decoding"]
    with pytest.raises(NotImplementedError, match="generation arguments together with ensemble_one_shots"):
        fx._generative_step(batch, 0, do_sample=True, seed=5)
    with pytest.raises(NotImplementedError, match="num_permutations_of_in_context_examples"):
        fx.answer_from_set(batch, _candidate_tensor(answers, 5))
    plain = fx._generative_step(batch, 0)["outputs"]
    want = fx.generate_from_ensembles(m["question_tokens"].to(DEV), m["question_mask"].to(DEV), m["prefix"].to(DEV), N, ML,
                                      sentinel=m["special_token_id"])
    assert [r.tolist() for r in plain] == [r.tolist() for r in want]


def test_executor_one_shot_ensembles_take_the_shot_and_the_query_image():
    """``ensemble_one_shots``: member i sees images ``[i, -1]`` and ``num_shots=1`` - the call ``generate_from_ensembles`` makes per member."""
    tag = "t0"
    z = sm.load_golden(f"vct0_{tag}.npz")
    V = int(z["cfg"][0])
    emb = torch.from_numpy(z["fs_prefix"])[:, :, 0]                                         # [B, 3, D]: two shots and the query image
    g = torch.Generator().manual_seed(4)
    tok = torch.randint(3, V - 10, (B, 2, 7), generator=g)
    tok[:, :, 1], tok[:, :, 4] = V - 1, V - 2                                               # one sentinel per image, in order
    mask = torch.ones_like(tok)
    batch = {"generative_input_ids": tok.reshape(B * 2, -1), "generative_attention_mask": mask.reshape(B * 2, -1), "clip_embeddings": emb}
    fx, few = _few_shot_executor(tag, ensemble_one_shots=True, num_shots=2, ensemble_decoding="select")
    got = fx._generative_step(batch, 0)["outputs"]
    del few.data_loader.additional["ensemble_decoding"]
    want = fx._generative_step(batch, 0)["outputs"]
    for b in range(B):
        assert _same_up_to_the_pad_tail(got[b], want[b], 0), (b, got[b], want[b])
    few.data_loader.additional.ensemble_decoding = "product"
    w = [0.0, 1.0]
    hot = fx.model.generate_ensemble(prefix=torch.stack([emb[:, [0, -1]], emb[:, [1, -1]]], dim=1), question_tokens=tok, question_mask=mask,
                                     ensemble="product", ensemble_weights=w, num_shots=1, max_length=ML, special_token_id=V - 1)
    solo = fx.model.generate(prefix=emb[:, [1, -1]], question_tokens=tok[:, 1], question_mask=mask[:, 1], num_shots=1, max_length=ML,
                             special_token_id=V - 1)
    assert torch.equal(hot, solo)
    assert fx._generative_step(batch, 0)["outputs"].shape == (B, ML)
