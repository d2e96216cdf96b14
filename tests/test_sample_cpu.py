"""CPU: ``eavqa_sample_pick`` validates its arguments before any launch, and the generation arguments of sampling are planned on the
host with HF's defaults - or named when they are not built."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


P = 4096      # a non-null, 16-byte aligned value standing in for a device pointer: every call below must return before it is used


def _pick(lib, **over):
    a = dict(B=2, V=32, logits=P, ld=32, temperature=1.0, top_k=0, top_p=1.0, seed=1, step=0, uniform_in=None, uniform_out=None, pad=0, eos=-1,
             raw=P, emitted=P, ld_emitted=1, unfinished=None, logprob=None, scores_out=None, ld_scores=0, any_unfinished=None)
    assert not set(over) - set(a), over
    a.update(over)
    return lib.eavqa_sample_pick(*a.values(), None)


def test_sample_pick_rejects_bad_arguments_before_any_launch(lib):
    for name in ("logits", "raw", "emitted"):
        assert _pick(lib, **{name: None}) == -1
    assert _pick(lib, B=0) == -1 and _pick(lib, B=-1) == -1 and _pick(lib, V=0) == -1
    assert _pick(lib, V=33) == -1                                          # ld < V
    assert _pick(lib, scores_out=P, ld_scores=31) == -1
    assert _pick(lib, eos=1) == -1                                         # an eos id needs the unfinished flags
    for t in (0.0, -1.0, float("inf"), float("nan")):
        assert _pick(lib, temperature=t) == -1
    for p in (0.0, -0.5, float("nan")):
        assert _pick(lib, top_p=p) == -1
    assert _pick(lib, V=65537, ld=65537) == -3                             # beyond what is built
    assert _pick(lib, V=65537, ld=65537, logits=None) == -1                # arguments before shape


def test_sample_pick_rejects_cpu_tensors():
    import torch
    from eavqa_amd import ops, _lib
    with pytest.raises(_lib.EavqaError, match="no CPU fallback"):
        ops.sample_pick(torch.zeros(2, 8), 8, 1.0, 0, 1.0, 1, 0, 0, None, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), None)


FIVE = dict(num_beams=1, num_return_sequences=1, length_penalty=1.0, early_stopping=False, eos_token_id=None)


def test_generation_plan_sampling_keys_and_defaults():
    from eavqa_amd.models.vct0 import generation_plan
    assert generation_plan({}) == FIVE and generation_plan(dict(do_sample=False)) == FIVE          # sampling keys only when sampling
    got = generation_plan(dict(do_sample=True))
    assert got == dict(FIVE, do_sample=True, temperature=1.0, top_k=50, top_p=1.0, seed=None)      # HF's defaults
    got = generation_plan(dict(do_sample=True, temperature=0.7, top_k=0, top_p=0.9, seed=11, num_return_sequences=8, eos_token_id=[3]))
    assert got == dict(FIVE, num_return_sequences=8, eos_token_id=3, do_sample=True, temperature=0.7, top_k=0, top_p=0.9, seed=11)
    assert generation_plan(dict(do_sample=True, top_k=None))["top_k"] == 0
    assert generation_plan(dict(do_sample=True), decoder_input_ids=object())["do_sample"]          # the decoder-prompt branch samples too


def test_generation_plan_names_what_sampling_does_not_build():
    from eavqa_amd.models.vct0 import generation_plan
    for name, value in (("top_p", 0.9), ("top_k", 5), ("temperature", 0.7)):
        with pytest.raises(NotImplementedError, match=name) as e:
            generation_plan({name: value})
        assert "greedy" in str(e.value)                                    # says why: no silent greedy run
    with pytest.raises(NotImplementedError, match="do_sample"):
        generation_plan(dict(do_sample=True, num_beams=2))
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        generation_plan(dict(do_sample=True, num_return_sequences=9))
    with pytest.raises(ValueError, match="num_return_sequences"):
        generation_plan(dict(do_sample=True, num_return_sequences=0))
    with pytest.raises(ValueError, match="num_return_sequences"):
        generation_plan(dict(num_return_sequences=2))                      # without sampling: <= num_beams, as before
    with pytest.raises(NotImplementedError, match="decoder_input_ids"):
        generation_plan(dict(do_sample=True, num_return_sequences=2), decoder_input_ids=object())
    for bad in (dict(temperature=0.0), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            generation_plan(dict(do_sample=True, **bad))


def test_causal_path_shares_the_plan_and_draws_repeatable_seeds():
    import torch
    from eavqa_amd.models import sampling

    class Owner:
        pass

    assert sampling.causal_sampler(Owner(), {}) is None and sampling.causal_sampler(Owner(), dict(do_sample=False)) is None
    s = sampling.causal_sampler(Owner(), dict(do_sample=True, seed=5))
    assert (s.temperature, s.top_k, s.top_p, s.seed) == (1.0, 50, 1.0, 5)
    with pytest.raises(NotImplementedError, match="top_p"):
        sampling.causal_sampler(Owner(), dict(top_p=0.9))
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        sampling.causal_sampler(Owner(), dict(do_sample=True, num_return_sequences=2))
    with pytest.raises(TypeError, match="num_beams"):
        sampling.causal_sampler(Owner(), dict(num_beams=2))
    # seed=None: torch.initial_seed() and a per-model call counter - torch.manual_seed makes a run repeatable, calls differ
    state = torch.random.get_rng_state()
    try:
        runs = []
        for _ in range(2):
            torch.manual_seed(1234)
            o = Owner()
            runs.append([sampling.causal_sampler(o, dict(do_sample=True)).seed for _ in range(3)])
        assert runs[0] == runs[1] and len(set(runs[0])) == 3 and all(0 <= v < 2 ** 64 for v in runs[0])
        torch.manual_seed(1235)
        assert sampling.causal_sampler(Owner(), dict(do_sample=True)).seed != runs[0][0]
    finally:
        torch.random.set_rng_state(state)


def test_the_beam_era_argument_checks_still_hold():
    from test_beam_cpu import test_generation_arguments_that_are_not_built_are_named
    test_generation_arguments_that_are_not_built_are_named()
