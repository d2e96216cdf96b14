"""GPU: ``ClipCaptionModel.score_candidates`` / ``score_candidates_fewshot`` (answer-candidate scoring behind a causal LM's prompt) on the
reference fixtures clipcap_gpt2_mlp.npz / clipcap_opt_mlp.npz (``gen_ids``, ``gen_mask`` with their padded rows, ``prefix``) against the CPU
oracle (``ref_cpu._prefix_inputs`` + ``ref_cpu.lm_logits`` on [prompt | candidate], in float64) put through tests/_score_ref.py; the shared
prompt cache against the replicated route; chunking bit for bit; the tie-in with greedy ``output_scores``; bf16 within twice the error
of the existing bf16 greedy path."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _score_ref as ref
from conftest import load_golden
from oracle import ref_cpu

DEV = "cuda"
MARGIN = 1e-3          # smallest gap between adjacent ranks a case may have (the project's constant: tests/test_beam_gpu.py)
ARCHS = [("gpt2", "clipcap_gpt2_mlp.npz"), ("opt", "clipcap_opt_mlp.npz")]
C, TC = 5, 4
T = torch.from_numpy


def _sub(z, prefix, double=False):
    return {k[len(prefix):]: (T(v).double() if double and v.dtype.kind == "f" else T(v)) for k, v in z.items() if k.startswith(prefix)}


@functools.lru_cache(maxsize=None)
def _fixture(arch):
    """(arrays, V, prefix length, CLIP width) of the fixture - no device needed."""
    z = load_golden(dict(ARCHS)[arch])
    return z, int(z["cfg"][0]), int(z["cfg"][5]), int(z["cfg"][6])


@functools.lru_cache(maxsize=None)
def _models(arch, dtype):
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig
    z = load_golden(dict(ARCHS)[arch])
    if arch == "gpt2":
        V, E, NLAY, NH, NPOS, L, D, CL, NL = [int(v) for v in z["cfg"]]
        cfg = LMConfig("gpt2", NLAY, NH, E, 4 * E, V, NPOS, 1e-5, "gelu_new", V - 1, None)
    else:
        V, E, NLAY, NH, NPOS, L, D, FFN = [int(v) for v in z["cfg"]]
        cfg = LMConfig("opt", NLAY, NH, E, FFN, V, NPOS, 1e-5, "relu", 2, 1)
    lm = FrozenCausalLM(cfg, _sub(z, "lm."), dtype, DEV)
    model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=DEV).eval()
    model.clip_project.load_state_dict(_sub(z, "map."), strict=True)
    return z, model, V, L, D


@functools.lru_cache(maxsize=None)
def _oracle(arch):
    z = load_golden(dict(ARCHS)[arch])
    return _sub(z, "lm.", True), dict(arch=arch, n_layer=int(z["cfg"][2]), n_head=int(z["cfg"][3])), _sub(z, "map.", True)


def _wte(sd, arch):
    return sd["transformer.wte.weight"] if arch == "gpt2" else sd["model.decoder.embed_tokens.weight"]


def _plain_prompt(arch):
    """The fixture's generation prompt: float64 (embeddings [B, L + T, E], attention mask) of [prefix | question], rows right-padded."""
    z, V, L, D = _fixture(arch)
    sd, cfg, mapper = _oracle(arch)
    with torch.no_grad():
        return ref_cpu._prefix_inputs(sd, cfg, mapper, dict(prefix_length=L, mapping_type="mlp"), T(z["gen_ids"]), T(z["prefix"]).double(),
                                      T(z["gen_mask"]).double())


def _fewshot_inputs(arch):
    """Three images per row, sentinel positions that differ between rows, right padding on one row (as tests/test_model_gpu.py)."""
    z, V, L, D = _fixture(arch)
    g = torch.Generator().manual_seed(9)
    B, n_img, seg = 3, 3, 4
    special = V - 5
    width = n_img * (1 + seg) + 2
    tok = torch.randint(3, special - n_img - 1, (B, width), generator=g)
    for b in range(B):
        for i in range(n_img):
            tok[b, i * (1 + seg) + (b % 2)] = special - i
    mask = torch.ones(B, width, dtype=torch.long)
    mask[1, -2:] = 0
    prefix = torch.randn(B, n_img, D, generator=g)
    return tok, mask, prefix, n_img, special


def _fewshot_prompt(arch):
    z, V, L, D = _fixture(arch)
    sd, cfg, mapper = _oracle(arch)
    tok, mask, prefix, n_img, special = _fewshot_inputs(arch)
    wte = _wte(sd, arch)
    with torch.no_grad():
        pp = ref_cpu.mlp_mapper(prefix.double().reshape(-1, D), mapper).reshape(tok.shape[0], n_img, L, wte.shape[1])
        emb, am = ref_cpu.insert_prefix_into_input(L, n_img - 1, tok, wte[tok], pp, mask, special_token_id=special)
    return emb, am.double()


def _oracle_logits(arch, prompt, cand):
    """float64 [B, C, Tc, V]: the oracle's next-token logits at every candidate position, from [prompt | candidate] per candidate."""
    sd, cfg, _ = _oracle(arch)
    emb, am = prompt
    B, Cn, Tn = cand.shape
    wte = _wte(sd, arch)
    S0 = emb.shape[1]
    with torch.no_grad():
        full = torch.cat([emb.repeat_interleave(Cn, dim=0), wte[cand.reshape(B * Cn, Tn).clamp_min(0)]], dim=1)
        mask = torch.cat([am.repeat_interleave(Cn, dim=0), torch.ones(B * Cn, Tn, dtype=am.dtype)], dim=1)
        logits = ref_cpu.lm_logits(sd, cfg, full, mask)[:, S0 - 1:S0 - 1 + Tn]
    return logits.reshape(B, Cn, Tn, -1).numpy()


def _candidates(V, B, seed, eos, n_cand=C, width=TC):
    """int64 [B, C, Tc], right-padded with -100: >= 1 content token in [3, V - 4) plus the eos, drawn per question."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.full((B, n_cand, width), ref.PAD, dtype=torch.int64)
    for b in range(B):
        for c in range(n_cand):
            n = int(torch.randint(1, width, (1,), generator=g))
            cand[b, c, :n] = torch.randint(3, V - 4, (n,), generator=g)
            cand[b, c, n] = eos
    return cand


def _check_against_oracle(arch, score, prompt, cand, monkeypatch, label):
    from eavqa_amd.models import scoring
    lp = ref.token_logprobs(_oracle_logits(arch, prompt, cand), cand.numpy())
    want, want_n, _ = ref.candidate_scores(lp, cand.numpy())
    gap = ref.min_rank_gap(want)
    assert gap >= MARGIN, f"test input: the oracle's smallest rank gap is {gap:.2e}"
    got = score(candidates=cand)
    err = np.abs(got.scores.cpu().numpy() - want).max()
    print(f"[{arch} {label}] oracle min gap {gap:.2e}; max |score - oracle| {err:.2e}")
    assert got.scores.shape == cand.shape[:2] and got.scores.dtype == torch.float32 and got.scores.is_cuda
    assert err <= 2e-4 and np.abs(got.token_logprobs.cpu().numpy() - lp).max() <= 2e-4
    assert (got.token_logprobs.cpu()[cand < 0] == 0).all() and np.array_equal(got.n_tokens.cpu().numpy(), want_n)
    assert np.array_equal(got.order.cpu().numpy(), ref.stable_order(want)) and torch.equal(got.best, got.order[:, 0])
    slow = score(candidates=cand, share_prompt=False)
    assert (slow.scores - got.scores).abs().max().item() <= 2e-4 and np.abs(slow.scores.cpu().numpy() - want).max() <= 2e-4
    assert torch.equal(slow.order, got.order)
    monkeypatch.setattr(scoring, "CHUNK_CANDIDATES", 1)
    for share, full in ((True, got), (False, slow)):
        one = score(candidates=cand, share_prompt=share)
        assert torch.equal(one.scores, full.scores) and torch.equal(one.token_logprobs, full.token_logprobs)
        assert torch.equal(one.order, full.order) and torch.equal(one.n_tokens, full.n_tokens)


def _plain_score(arch, dtype):
    z, model, V, L, D = _models(arch, dtype)
    return lambda **kw: model.score_candidates(T(z["gen_ids"]), T(z["prefix"]), T(z["gen_mask"]), **kw)


def _fewshot_score(arch, dtype):
    _, model, V, L, D = _models(arch, dtype)
    tok, mask, prefix, n_img, special = _fewshot_inputs(arch)
    return lambda **kw: model.score_candidates_fewshot(tok, prefix, mask, num_shots=n_img - 1, special_token_id=special, **kw)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_scores_and_ranking_match_the_oracle_behind_the_fixture_prompt(arch, seed, monkeypatch):
    z, model, V, L, D = _models(arch, torch.float32)
    assert (z["gen_mask"] == 0).any()                                           # the fixture does hold padded prompt rows
    cand = _candidates(V, z["gen_ids"].shape[0], seed, model.gpt.cfg.eos_token_id)
    _check_against_oracle(arch, _plain_score(arch, torch.float32), _plain_prompt(arch), cand, monkeypatch, f"plain seed {seed}")


@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_fewshot_scores_and_ranking_match_the_oracle(arch, monkeypatch):
    z, model, V, L, D = _models(arch, torch.float32)
    cand = _candidates(V, 3, 2, model.gpt.cfg.eos_token_id)
    _check_against_oracle(arch, _fewshot_score(arch, torch.float32), _fewshot_prompt(arch), cand, monkeypatch, "few-shot")


def test_single_token_candidates_shared_list_and_host_errors():
    """Tc = 1 (yes / no style answers): only the prefill's last-position logits are used; a [C, Tc] list serves every question."""
    z, model, V, L, D = _models("gpt2", torch.float32)
    score = _plain_score("gpt2", torch.float32)
    shared = torch.tensor([[5], [9], [V - 1], [40]])
    B = z["gen_ids"].shape[0]
    cand = shared[None].expand(B, -1, -1).contiguous()
    lp = ref.token_logprobs(_oracle_logits("gpt2", _plain_prompt("gpt2"), cand), cand.numpy())
    for share in (True, False):
        got = score(candidates=shared, share_prompt=share)
        assert np.abs(got.scores.cpu().numpy() - lp[..., 0]).max() <= 2e-4 and (got.n_tokens == 1).all()
    got = score(candidates=shared, ignored_ids=(V - 1,), length_penalty=1.0)
    assert torch.isneginf(got.scores[:, 2]).all() and (got.order[:, -1] == 2).all() and (got.n_tokens[:, 2] == 0).all()
    with pytest.raises(ValueError, match="without a token"):
        score(candidates=torch.tensor([[5, 6], [-100, -100]]))
    with pytest.raises(TypeError, match="top_k"):
        score(candidates=shared, top_k=3)


def _greedy_case(arch, dtype, fewshot):
    """(candidates [B, 1, n] = the greedy ids, float64 sums of the greedy ``output_scores`` log-probabilities, prompt, score function)."""
    z, model, V, L, D = _models(arch, dtype)
    pad = int(z["pad_id"])
    if fewshot:
        tok, mask, prefix, n_img, special = _fewshot_inputs(arch)
        ids, lp = model.generate_fewshot(tok, prefix, mask, num_shots=n_img - 1, special_token_id=special, max_length=5, pad_token_id=pad,
                                         eos_token_id=None, output_scores=True)
        return T(np.asarray(ids))[:, None, :], lp.double().sum(1).numpy(), _fewshot_prompt(arch), _fewshot_score(arch, dtype)
    ids, lp = model.generate(T(z["gen_ids"]), T(z["prefix"]), T(z["gen_mask"]), max_length=5, pad_token_id=pad, eos_token_id=None, output_scores=True)
    return T(np.asarray(ids))[:, None, :], lp.double().sum(1).numpy(), _plain_prompt(arch), _plain_score(arch, dtype)


@pytest.mark.parametrize("fewshot", [False, True])
@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_the_greedy_sequence_scores_what_generate_reported_and_ranks_first(arch, fewshot):
    cand, sums, prompt, score = _greedy_case(arch, torch.float32, fewshot)
    B, _, n = cand.shape
    step = torch.log_softmax(T(_oracle_logits(arch, prompt, cand))[:, 0, n - 1], dim=-1)          # the oracle's distribution of the last step
    pair = cand.repeat(1, 2, 1)
    for b in range(B):                                                          # the last token swapped for the least likely one of its step
        worst = int(step[b].argmin())
        assert float(step[b, worst]) < float(step[b, cand[b, 0, n - 1]]) - MARGIN
        pair[b, 1, n - 1] = worst
    got = score(candidates=pair)
    err = np.abs(got.scores[:, 0].cpu().numpy() - sums).max()
    print(f"[{arch} fewshot={fewshot}] greedy sequences of {n} tokens: max |score - sum of output_scores| {err:.2e}")
    assert err <= 2e-4
    assert got.best.tolist() == [0] * B and (got.scores[:, 0] > got.scores[:, 1]).all()


def test_bf16_scores_stay_within_twice_the_error_of_the_bf16_greedy_path():
    """The tolerance cannot be derived, so it is measured: per fixture, the existing bf16 greedy path's sum of ``output_scores``
    log-probabilities at the emitted ids (plain and few-shot prompt) deviates from the float64 oracle's score of the same sequence by some
    figure; the new path (same arithmetic, another batching) may deviate from the oracle by at most twice the largest such figure, for
    the greedy sequences and for the random candidates, under both sharing schemes.
    Measured on MI355X (also in profiles/answer_scoring.md): gpt2 greedy path 3.994e-03, score_candidates 4.076e-03 (bound 7.988e-03); opt
    greedy path 3.551e-03, score_candidates 3.729e-03 (bound 7.102e-03)."""
    for arch in ("gpt2", "opt"):
        _, model, V, L, D = _models(arch, torch.bfloat16)
        greedy_err, new_err = 0.0, 0.0
        for fewshot in (False, True):
            cand, sums, prompt, score = _greedy_case(arch, torch.bfloat16, fewshot)
            rnd = _candidates(V, cand.shape[0], 0, model.gpt.cfg.eos_token_id)
            for cnd, given in ((cand, sums), (rnd, None)):
                want, _, _ = ref.candidate_scores(ref.token_logprobs(_oracle_logits(arch, prompt, cnd), cnd.numpy()), cnd.numpy())
                if given is not None:
                    greedy_err = max(greedy_err, float(np.abs(given - want[:, 0]).max()))
                for share in (True, False):
                    got = score(candidates=cnd, share_prompt=share).scores.cpu().numpy()
                    new_err = max(new_err, float(np.abs(got - want).max()))
        print(f"[{arch} bf16] greedy path |sum of output_scores - oracle| {greedy_err:.3e}; score_candidates |score - oracle| {new_err:.3e}")
        assert new_err <= 2 * greedy_err
