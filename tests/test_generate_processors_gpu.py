"""GPU: ``generate`` under HF's logits processors (``repetition_penalty``, ``no_repeat_ngram_size``, ``min_length``, ``min_new_tokens``,
``bad_words_ids``) end to end: the T5 path against what the REFERENCE's ``VCT0Prefix.generate`` produced (tests/golden/vct0_logits.npz,
written by tests/golden/make_golden_logits.py), sampling reduced to one token against the same ids, the causal path against a host loop
over the oracle's logits and tests/_logits_ref.py, and the no-op guarantee: without a processor argument nothing new is launched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _logits_ref as ref
from conftest import load_golden

DEV = "cuda"
MARGIN = 1e-3


def T(a):
    return torch.from_numpy(a)


def _fixture_call(z, tag, name, path, V):
    f = lambda field: z[f"{tag}.{name}.{field}"]
    k, max_length, eos, ngram, min_length, min_new = [int(v) for v in f("params")]
    kw = dict(max_length=max_length, special_token_id=V - 1)
    if eos >= 0:
        kw["eos_token_id"] = eos
    rp = float(f("repetition_penalty"))
    proc = {}
    if rp != 1.0:
        proc["repetition_penalty"] = rp
    if ngram:
        proc["no_repeat_ngram_size"] = ngram
    if min_length:
        proc["min_length"] = min_length
    if min_new:
        proc["min_new_tokens"] = min_new
    words = [[int(t) for t in w if t >= 0] for w in f("bad_words")]
    if words:
        proc["bad_words_ids"] = words
    inputs = dict(prefix=T(f("prefix"))) if path == "prefix" else dict(prefix=T(f("prefix")), question_tokens=T(f("tokens")),
                                                                        question_mask=T(f("mask")))
    return k, dict(inputs, **kw), proc, f


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("tag", ["t0", "t5v10"])
def test_t5_generate_with_processors_matches_the_reference(tag, native):
    """Every case of vct0_logits.npz in fp32, cached and ``use_cache=False``: ids exact (shape included); beams also
    ``sequences_scores`` within 2e-4, the tolerance of the beam fixture test (2e-5 logits parity x at most 7 accumulated steps)."""
    from test_beam_gpu import _model
    z = load_golden("vct0_logits.npz")
    model, V, D = _model(tag, torch.float32)
    model.lm.native_step = native
    for name, path in zip(z["cases"].tolist(), z["paths"].tolist()):
        k, kw, proc, f = _fixture_call(z, tag, name, path, V)
        assert float(f("min_gap")) >= MARGIN and proc
        want = T(f("sequences"))
        for use_cache in (True, False):
            if k > 1:
                o = model.generate(num_beams=k, num_return_sequences=k, output_scores=True, return_dict_in_generate=True, use_cache=use_cache,
                                   **kw, **proc)
                err = (o.sequences_scores - T(f("sequences_scores"))).abs().max().item()
                print(f"[{tag} {name} native={native} cache={use_cache}] max |score diff| {err:.2e}")
                assert o.sequences.shape == want.shape and torch.equal(o.sequences, want), (name, use_cache, o.sequences, want)
                assert err <= 2e-4, (name, use_cache)
            else:
                got = model.generate(use_cache=use_cache, **kw, **proc)
                assert got.shape == want.shape and torch.equal(got, want), (name, use_cache, got, want)
        if k == 1:                                                          # without the arguments: the fixture's other run
            plain = model.generate(**kw)
            assert plain.shape == T(f("plain")).shape and torch.equal(plain, T(f("plain"))), name


def test_output_scores_are_the_processed_scores():
    """HF's ``.scores`` under greedy search hold the processed row: -inf at what a rule banned."""
    from test_beam_gpu import _model
    z = load_golden("vct0_logits.npz")
    model, V, D = _model("t0", torch.float32)
    k, kw, proc, f = _fixture_call(z, "t0", "g_ng1", "fs", V)
    o = model.generate(output_scores=True, return_dict_in_generate=True, **kw, **proc)
    assert torch.equal(o.sequences, T(f("sequences")))
    for j, s in enumerate(o.scores):
        for r in range(s.shape[0]):
            seen = o.sequences[r, :j + 1]
            assert (s[r, seen] == float("-inf")).all() and int(torch.isinf(s[r]).sum()) == len(set(seen.tolist()))


@pytest.mark.parametrize("tag", ["t0", "t5v10"])
def test_sampling_that_leaves_one_token_reproduces_the_greedy_cases(tag):
    from test_beam_gpu import _model
    z = load_golden("vct0_logits.npz")
    model, V, D = _model(tag, torch.float32)
    for name, path in zip(z["cases"].tolist(), z["paths"].tolist()):
        k, kw, proc, f = _fixture_call(z, tag, name, path, V)
        if k == 1:
            got = model.generate(do_sample=True, top_k=1, seed=5, **kw, **proc)
            assert torch.equal(got, T(f("sequences"))), name


@pytest.mark.parametrize("nrs", [1, 4])
def test_free_sampling_without_repeats_returns_distinct_tokens(nrs):
    from test_beam_gpu import _model
    z = load_golden("vct0_logits.npz")
    model, V, D = _model("t0", torch.float32)
    k, kw, proc, f = _fixture_call(z, "t0", "g_ng1", "fs", V)
    got = model.generate(do_sample=True, top_k=0, temperature=1.5, seed=11, num_return_sequences=nrs, no_repeat_ngram_size=1, **kw)
    assert got.shape[0] == 3 * nrs
    for row in got.tolist():
        body = row[:row.index(1, 1)] if 1 in row[1:] else row            # up to the first eos (the start token 0 counts as seen)
        assert len(set(body)) == len(body), row


# ------------------------------------------------------------------------------------------------ the causal path
def _oracle_ids(z, arch, max_length, eos, pad, **rules):
    """Greedy ids of a host loop: oracle logits -> tests/_logits_ref.py -> arg-max -> append, with the bookkeeping of the reference's
    loop (a row that emitted ``eos`` emits ``pad`` from then on; the embedding fed back is the raw arg-max; stop when every row has
    finished).  The history the rules see is what was emitted.  Returns (ids, smallest top-1 / top-2 gap over unfinished rows)."""
    from oracle import ref_cpu
    from test_model_gpu import sub
    c = [int(v) for v in z["cfg"]]
    cfg = dict(arch=arch, n_layer=c[2], n_head=c[3])
    mcfg = dict(prefix_length=c[5], clip_length=c[7] if arch == "gpt2" else None, num_layers=c[8] if arch == "gpt2" else 8, mapping_type="mlp")
    sd = sub(z, "lm.")
    with torch.no_grad():
        emb, am = ref_cpu._prefix_inputs(sd, cfg, sub(z, "map."), mcfg, T(z["gen_ids"]), T(z["prefix"]), T(z["gen_mask"]))
        wte = ref_cpu._wte(sd, cfg)
        B = emb.shape[0]
        tokens = torch.zeros((B, 0), dtype=torch.int64)
        unfinished = torch.ones(B, dtype=torch.bool)
        gap = float("inf")
        for _ in range(max_length):
            logits = ref_cpu.lm_logits(sd, cfg, emb, am)[:, -1, :].float()
            s = ref.process(logits, tokens, **rules)
            top = torch.sort(s, dim=-1, descending=True).values[unfinished, :2]
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
            nxt = torch.argmax(s, -1)
            emitted = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            tokens = torch.cat([tokens, emitted[:, None]], dim=1)
            emb = torch.cat((emb, wte[nxt[:, None]]), dim=1)
            am = torch.cat([am, torch.ones((B, 1))], dim=-1)
            unfinished = unfinished & (emitted != eos)
            if not unfinished.any():
                break
    return tokens.tolist(), gap


@pytest.mark.parametrize("arch,fixture", [("gpt2", "clipcap_gpt2_mlp.npz"), ("opt", "clipcap_opt_mlp.npz")])
def test_causal_generate_with_processors_matches_the_oracle_loop(arch, fixture):
    """``eos_token_id=None`` on the call: the config's eos id holds, as in the existing generate tests."""
    from test_model_gpu import build_model
    z = load_golden(fixture)
    model = build_model(z, arch, "mlp", torch.float32).eval()
    eos, pad = model.gpt.cfg.eos_token_id, int(z["pad_id"])
    want, gap = _oracle_ids(z, arch, 6, eos, pad, no_repeat_ngram_size=2, repetition_penalty=1.3)
    plain, _ = _oracle_ids(z, arch, 6, eos, pad)
    print(f"[{arch}] smallest oracle gap {gap:.2e}")
    assert gap >= MARGIN, gap                                     # a smaller gap is a test-input error: the case fails
    assert want != plain                                          # the rules act on these inputs
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=6,
              pad_token_id=pad, eos_token_id=None, no_repeat_ngram_size=2, repetition_penalty=1.3)
    assert model.generate(**{**kw, "no_repeat_ngram_size": None, "repetition_penalty": None}) == plain
    for use_cache in (True, False):
        assert model.generate(use_cache=use_cache, **kw) == want, use_cache
    # sampling reduced to one token takes the same route; the log-probability under the processed distribution is log 1
    ids, lp = model.generate(do_sample=True, top_k=1, seed=3, output_scores=True, **kw)
    assert ids == want and (lp == 0).all()
    with pytest.raises(TypeError, match="num_beams"):             # unknown names are still rejected by name
        model.generate(num_beams=2, **kw)
    with pytest.raises(ValueError, match="min_length"):
        model.generate(min_length=7, **kw)                        # above max_length
    bf = build_model(z, arch, "mlp", torch.bfloat16).eval()
    assert bf.generate(use_cache=True, **kw) == bf.generate(use_cache=False, **kw)


@pytest.mark.parametrize("arch,fixture", [("gpt2", "clipcap_gpt2_mlp.npz"), ("opt", "clipcap_opt_mlp.npz")])
def test_causal_generate_never_emits_a_banned_first_token(arch, fixture):
    """The first causal step has an EMPTY history (with ``inputs_embeds`` HF's ``input_ids`` start empty), and a one-token bad word bans
    there too: the words are the very tokens the plain run emits first.  Then two-token words made of what the banned run repeats: HF
    skips a word longer than the history, so ``[x, x]`` lets the second x through and bans the third.  ``max_length`` 4: on these
    fixtures every oracle gap of both runs is >= 1e-3 there (asserted; a smaller gap is a test-input error and fails)."""
    from test_model_gpu import build_model
    z = load_golden(fixture)
    model = build_model(z, arch, "mlp", torch.float32).eval()
    eos, pad = model.gpt.cfg.eos_token_id, int(z["pad_id"])
    plain, _ = _oracle_ids(z, arch, 4, eos, pad)
    first = sorted({row[0] for row in plain} - {eos})             # (an [eos] word would be dropped; a row that starts with eos stays)
    live = [i for i, row in enumerate(plain) if row[0] != eos]
    assert len(live) >= 2
    single = [[t] for t in first]
    banned, gap1 = _oracle_ids(z, arch, 4, eos, pad, bad_words=single)
    double = single + [list(p) for p in sorted({(banned[i][0], banned[i][1]) for i in live})]
    want, gap2 = _oracle_ids(z, arch, 4, eos, pad, bad_words=double)
    print(f"[{arch}] smallest oracle gaps {gap1:.2e} {gap2:.2e}")
    assert min(gap1, gap2) >= MARGIN, (gap1, gap2)
    assert all(banned[i][0] not in first + [eos] for i in live) and want != banned
    assert all(want[i][:2] == banned[i][:2] and want[i][2] != want[i][1] for i in live)
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=4,
              pad_token_id=pad, eos_token_id=None)
    assert model.generate(**kw) == plain
    for use_cache in (True, False):
        assert model.generate(use_cache=use_cache, bad_words_ids=single, **kw) == banned, use_cache
        assert model.generate(use_cache=use_cache, bad_words_ids=double, **kw) == want, use_cache
    assert model.generate(bad_words_ids=[[np.int64(t) for t in w] for w in double], **kw) == want          # ids as a fixture holds them
    assert model.generate(do_sample=True, top_k=1, seed=3, bad_words_ids=single, **kw) == banned


# ------------------------------------------------------------------------------------------------ no processor argument: nothing new runs
def test_without_processor_arguments_logits_process_is_never_called(monkeypatch):
    from eavqa_amd import ops
    from test_beam_gpu import _model
    from test_model_gpu import build_model
    calls = []
    real = ops.logits_process
    monkeypatch.setattr(ops, "logits_process", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    z = load_golden("vct0_beam.npz")
    model, V, D = _model("t0", torch.float32)
    f = lambda field: T(z[f"t0.fs_k3.{field}"])
    k, nrs, es, eos, max_length = [int(v) for v in f("params")]
    kw = dict(prefix=f("prefix"), question_tokens=f("tokens"), question_mask=f("mask"), max_length=max_length, special_token_id=V - 1, eos_token_id=eos)
    assert torch.equal(model.generate(**kw), f("greedy"))                                                       # greedy
    assert torch.equal(model.generate(num_beams=k, num_return_sequences=nrs, **kw), f("sequences"))            # beams
    assert torch.equal(model.generate(do_sample=True, top_k=1, **kw), f("greedy"))                              # sampling
    assert torch.equal(model.generate(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, **kw), f("greedy"))
    zc = load_golden("clipcap_gpt2_mlp.npz")
    causal = build_model(zc, "gpt2", "mlp", torch.float32).eval()
    ckw = dict(question_tokens=T(zc["gen_ids"]), prefix=T(zc["prefix"]), question_mask=T(zc["gen_mask"]), max_length=6,
               pad_token_id=int(zc["pad_id"]), eos_token_id=None)
    assert causal.generate(**ckw) == zc["gen_free"].tolist()                                                    # the causal loop
    assert causal.generate(repetition_penalty=1.0, **ckw) == zc["gen_free"].tolist()
    assert not calls
    got = model.generate(no_repeat_ngram_size=2, **kw)
    # one call per step the loop ran: a step per id after the start token, up to the next look at the stop flag (every fourth step)
    assert len(calls) == min(max_length - 1, -(-(got.shape[1] - 1) // 4) * 4), (len(calls), got.shape)
