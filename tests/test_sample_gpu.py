"""GPU: ``eavqa_sample_pick`` against the HF restatement of tests/_sampling_ref.py (filters, inverse CDF with given uniforms, Philox,
the drawn distribution, finished-row bookkeeping), and sampling through ``VCT0Prefix.generate`` / ``ClipCaptionPrefix.generate`` on
the reference's tiny fixtures: settings that leave one token must reproduce the greedy ids, and a free run must be the inverse CDF
of its own returned scores under the reference Philox."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sampling_ref as R
from conftest import GOLDEN

DEV = "cuda"
PAD_FILL = 3.0e38          # what the columns >= V hold: one read of them and the maximum (so every kept value) is wrong
SENTINEL = 123.0           # what scores_out holds beyond column V before the call: must still be there afterwards


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


def pick(ops, logits, ld=None, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0, uniform=None, eos=None, pad=0, unfinished=None,
         scores=True, want_uniform=False):
    """One launch on float32 CPU ``logits`` [B, V] placed in a [B, ld] device buffer; every output back on the host."""
    B, V = logits.shape
    ld = V if ld is None else ld
    buf = torch.full((B, ld), PAD_FILL, dtype=torch.float32)
    buf[:, :V] = logits
    buf = buf.to(DEV)
    raw = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    emitted = torch.full((B, 3), -7, dtype=torch.int64, device=DEV)
    unf = (torch.ones(B, dtype=torch.int32) if unfinished is None else unfinished.to(torch.int32)).to(DEV)
    alive = torch.zeros(1, dtype=torch.int32, device=DEV)
    lp = torch.full((B,), 9.0, dtype=torch.float32, device=DEV)
    so = torch.full((B, ld), SENTINEL, dtype=torch.float32, device=DEV) if scores else None
    uo = torch.full((B,), -1.0, dtype=torch.float32, device=DEV) if want_uniform else None
    ui = torch.as_tensor(np.asarray(uniform, dtype=np.float32)).to(DEV) if uniform is not None else None
    ops.sample_pick(buf, V, temperature, top_k, top_p, seed, step, pad, eos, raw, emitted[:, 1], unf, lp, alive if eos is not None else None,
                    scores_out=so, uniform_in=ui, uniform_out=uo)
    torch.cuda.synchronize()
    out = dict(raw=raw.cpu(), emitted=emitted.cpu(), unfinished=unf.cpu(), alive=int(alive.item()), logprob=lp.cpu(),
               scores=so.cpu() if scores else None, uniform=uo.cpu().numpy() if want_uniform else None)
    assert ((out["raw"] >= 0) & (out["raw"] < V)).all()
    assert (out["emitted"][:, 0] == -7).all() and (out["emitted"][:, 2] == -7).all()          # the emitted column only
    return out


# ------------------------------------------------------------------------------------------------ 1. filters
@pytest.mark.parametrize("B,V,ld", R.SHAPES, ids=[f"B{b}-V{v}-ld{l}" for b, v, l in R.SHAPES])
def test_filter_set_equals_the_reference_exactly(ops, B, V, ld):
    """V = 7: fewer columns than a wave; 64; 1000 with ld 1001: the scalar-load path; 32 128 with ld 32 192: 16-byte loads and padding;
    50 272: more than 32 values per thread.  Over temperature x top_k x top_p: the finite mask of scores_out IS the reference's, kept
    values are logits / temperature in fp32, the drawn token is a kept one and its logprob is that of the reference distribution."""
    x = R.case_logits(B, V)
    n = 0
    for b_, v_, _, t, k, p in R.filter_cases():
        if (b_, v_) != (B, V):
            continue
        want = R.warp(x, t, k, p)
        got = pick(ops, x, ld, t, k, p, seed=n, step=3)
        s = got["scores"]
        assert torch.equal(torch.isfinite(s[:, :V]), torch.isfinite(want)), (t, k, p)
        keep = torch.isfinite(want)
        assert torch.equal(s[:, :V][keep], want[keep]), (t, k, p)
        assert (s[:, :V][~keep] == R.NEG_INF).all() and (s[:, V:] == SENTINEL).all(), (t, k, p)
        for b in range(B):
            i = int(got["raw"][b])
            assert keep[b, i], (t, k, p, b, i)
            assert abs(float(got["logprob"][b]) - math.log(float(R.probs(want[b])[i]))) <= 2e-5, (t, k, p, b)
        n += 1
    assert n == len(R.TEMPERATURES) * len(R.TOP_KS) * len(R.TOP_PS)


def test_all_equal_row_keeps_every_token_under_top_k(ops):
    """HF's tie rule: ties with the top_k-th value all stay."""
    for V in (64, 1000):
        got = pick(ops, torch.full((2, V), 0.25), V + 1, top_k=3)
        assert torch.equal(got["scores"][:, :V], torch.full((2, V), 0.25))
        assert (got["logprob"] - math.log(1.0 / V)).abs().max().item() <= 2e-5


DENSE = [(2, 32128, 32192), (1, 50272, 50272)]
BAND = 1e-5      # fp32 tree sums of <= 65 536 positive terms: <= ~80 roundings of 2^-24 relative on the longest path, 5e-6


@pytest.mark.parametrize("B,V,ld", DENSE, ids=[f"B{b}-V{v}" for b, v, _ in DENSE])
def test_dense_rows_match_outside_the_rounding_band(ops, B, V, ld):
    """Every column finite, as an LM head's logits: a top-p boundary then lies within ~1e-5 of some token's cumulative probability, so
    tokens within BAND of the boundary (float64, reference only) may fall either side; every other token must match, the kept set must
    be a value threshold, and top-k (integer counts) must match exactly."""
    x = R.dense_logits(B, V)
    for t in R.TEMPERATURES:
        for k in (0, 50):
            for p in (1.0, 0.9, 0.5):
                want = R.warp(x, t, k, p)
                s = pick(ops, x, ld, t, k, p, seed=5)["scores"][:, :V]
                for b in range(B):
                    band = R.top_p_band(x[b], t, k, p, BAND) if p < 1.0 else torch.zeros(V, dtype=torch.bool)
                    assert int(band.sum()) <= 8, (t, k, p, int(band.sum()))
                    same = torch.isfinite(s[b]) == torch.isfinite(want[b])
                    assert same[~band].all(), (t, k, p, b, int((~same).sum()))
                    kept = torch.isfinite(s[b])
                    assert torch.equal(s[b][kept], (x[b] / torch.tensor(t))[kept])
                    gone = ~kept & torch.isfinite(x[b])
                    if gone.any():
                        assert s[b][kept].min() > (x[b] / torch.tensor(t))[gone].max(), (t, k, p, b)


# ------------------------------------------------------------------------------------------------ 2. the draw, given uniforms
DRAW_SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 0.9), (2.0, 0, 0.5), (1.0, 2, 1.0)]


def _targets(row_processed, n):
    """Up to n target tokens with p >= 1e-4, spread over the kept set in index order (first and last of them included)."""
    ok = (R.probs(row_processed) >= 1e-4).nonzero().flatten().tolist()
    if len(ok) <= n:
        return ok
    return [ok[round(j * (len(ok) - 1) / (n - 1))] for j in range(n)]


@pytest.mark.parametrize("B,V,ld", R.SHAPES + DENSE[:1], ids=[f"B{b}-V{v}-ld{l}" for b, v, l in R.SHAPES + DENSE[:1]])
def test_draw_is_the_inverse_cdf_of_the_given_uniform(ops, B, V, ld):
    dense = ld == 32192 and B == 2
    x = R.dense_logits(B, V) if dense else R.case_logits(B, V)
    for t, k, p in DRAW_SETTINGS[:1] + [(0.7, 50, 1.0)] if dense else DRAW_SETTINGS:
        proc = R.warp(x, t, k, p)
        targets = [_targets(proc[b], 4) for b in range(B)]
        for j in range(4):
            want = [tg[min(j, len(tg) - 1)] for tg in targets]
            u = [R.midpoint_uniform(proc[b], want[b]) for b in range(B)]
            got = pick(ops, x, ld, t, k, p, uniform=u, scores=False, want_uniform=True)
            assert got["raw"].tolist() == want, (t, k, p, j)
            assert np.array_equal(got["uniform"], np.asarray(u, dtype=np.float32))
            for b in range(B):
                assert abs(float(got["logprob"][b]) - math.log(float(R.probs(proc[b])[want[b]]))) <= 2e-5, (t, k, p, b)
        if dense:
            continue
        mass = [(R.probs(proc[b]) > 0).nonzero().flatten() for b in range(B)]
        first, last = [int(m[0]) for m in mass], [int(m[-1]) for m in mass]
        assert pick(ops, x, ld, t, k, p, uniform=[0.0] * B, scores=False)["raw"].tolist() == first, (t, k, p)
        # u = 1 - 2^-24 reaches the last kept token when that token weighs more than 2^-24 (and fp32 slack): the fixed cases do
        assert min(float(R.probs(proc[b])[last[b]]) for b in range(B)) >= 1e-5, (t, k, p)
        assert pick(ops, x, ld, t, k, p, uniform=[1.0 - 2.0 ** -24] * B, scores=False)["raw"].tolist() == last, (t, k, p)


def test_never_an_index_outside_the_row(ops):
    """No finite entry, NaNs, +inf, and uniforms outside [0, 1): the index stays in [0, V) (checked in ``pick``) and holds mass."""
    V = 1000
    x = torch.full((4, V), R.NEG_INF)
    x[1, 5] = float("nan")
    x[2, :] = float("nan")
    x[2, 17] = 0.5
    x[3, 900] = float("inf")
    x[3, 3] = 2.0
    for u in ([0.3] * 4, [1.0, 2.0, float("nan"), -1.0]):
        got = pick(ops, x, V + 1, uniform=u, top_k=50, top_p=0.9)
        assert int(got["raw"][2]) == 17 and int(got["raw"][3]) == 900


# ------------------------------------------------------------------------------------------------ 3. Philox
def test_philox_uniforms_are_the_reference_bit_for_bit(ops):
    B, V = 5, 1000
    x = R.case_logits(B, V)
    for seed in (1, (1 << 40) + 12345):
        for step in (0, (1 << 33) + 5):
            a = pick(ops, x, V + 1, 0.7, 0, 1.0, seed=seed, step=step, want_uniform=True)
            assert np.array_equal(a["uniform"].view(np.uint32), R.philox_uniforms(seed, step, B).view(np.uint32)), (seed, step)
            b = pick(ops, x, V + 1, 0.7, 0, 1.0, seed=99, step=1, uniform=a["uniform"])
            assert torch.equal(a["raw"], b["raw"]) and torch.equal(a["logprob"], b["logprob"])
            c = pick(ops, x, V + 1, 0.7, 0, 1.0, seed=seed, step=step, want_uniform=True)
            for name in ("raw", "emitted", "unfinished", "logprob", "scores"):
                assert torch.equal(a[name].view(torch.int32) if a[name].dtype == torch.float32 else a[name],
                                   c[name].view(torch.int32) if c[name].dtype == torch.float32 else c[name]), name
            assert np.array_equal(a["uniform"].view(np.uint32), c["uniform"].view(np.uint32))


def test_two_launches_are_bit_identical_on_a_dense_row(ops):
    x = R.dense_logits(2, 50272)
    a, b = (pick(ops, x, 50272, 0.7, 50, 0.9, seed=3, step=2) for _ in range(2))
    for name in ("raw", "logprob", "scores"):
        assert torch.equal(a[name].view(torch.int32) if a[name].dtype == torch.float32 else a[name],
                           b[name].view(torch.int32) if b[name].dtype == torch.float32 else b[name]), name


# ------------------------------------------------------------------------------------------------ 4. the distribution
def _chi_square(counts, p):
    n = counts.sum()
    live = p > 0
    return float((((counts[live] - n * p[live]) ** 2) / (n * p[live])).sum())


def test_drawn_distribution_is_the_reference_distribution(ops):
    """4 096 rows of the same 8 logits, one launch, Philox uniforms of a fixed seed (so the outcome is deterministic).  Pearson
    chi-square against the reference probabilities below the 1 - 1e-6 quantile: 40.5 at 7 degrees of freedom; with top_k = 3 two
    degrees of freedom, whose quantile is -2 ln(1e-6) = 27.63 (chi-square with 2 degrees is exponential)."""
    row = torch.tensor([0.0, 1.0, -1.0, 0.5, 2.0, -0.5, 1.5, 0.2])
    x = row[None].repeat(4096, 1)
    for top_k, bound in ((0, 40.5), (3, 27.63)):
        got = pick(ops, x, 8, 1.0, top_k, 1.0, seed=20261018, step=1, scores=False)
        p = R.probs(R.warp(row[None], 1.0, top_k, 1.0)[0]).numpy()
        counts = np.bincount(got["raw"].numpy(), minlength=8).astype(np.float64)
        assert counts[p == 0].sum() == 0                                   # a removed token is never drawn
        chi = _chi_square(counts, p)
        print(f"top_k={top_k}: chi-square {chi:.2f} (bound {bound})")
        assert chi < bound, (top_k, chi)
        assert len(set(got["raw"].tolist())) == (8 if top_k == 0 else 3)


# ------------------------------------------------------------------------------------------------ 5. bookkeeping
def test_finished_row_bookkeeping_is_greedy_picks_under_top_k_1(ops):
    B, V = 6, 1000
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(4)) * 3
    eos = int(x[1].argmax())
    unf0 = torch.tensor([1, 1, 0, 1, 0, 1])
    for unf_in, want_alive in ((unf0, 1), (torch.tensor([0, 1, 0, 0, 0, 0]), 0)):
        got = pick(ops, x, V, 0.7, 1, 1.0, eos=eos, pad=42, unfinished=unf_in, scores=False)
        buf = x.to(DEV)
        raw = torch.empty(B, dtype=torch.int32, device=DEV)
        em = torch.zeros(B, 3, dtype=torch.int64, device=DEV)
        unf = unf_in.to(torch.int32).to(DEV)
        alive = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.greedy_pick(buf, V, 42, eos, raw, em[:, 1], unf, None, alive)
        assert torch.equal(got["raw"], raw.cpu()) and torch.equal(got["emitted"][:, 1], em[:, 1].cpu())
        assert torch.equal(got["unfinished"], unf.cpu()) and got["alive"] == int(alive.item()) == want_alive
        assert (got["logprob"] == 0).all()                                 # one token left: log 1
    free = pick(ops, x, V, 0.7, 1, 1.0, eos=None, unfinished=unf0, scores=False)      # eos None: raw tokens, flags untouched
    assert torch.equal(free["emitted"][:, 1], free["raw"].long()) and torch.equal(free["unfinished"], unf0.int())


# ------------------------------------------------------------------------------------------------ 6. models: one token left = greedy
ONE_TOKEN = [dict(top_k=1), dict(top_p=1e-6, top_k=0), dict(temperature=0.5, top_k=1)]


@pytest.mark.parametrize("tag", ["t0", "t5v10"])
def test_vct0_sampling_that_leaves_one_token_returns_the_fixture_greedy_ids(tag):
    """The reference's own greedy ids (tests/golden/vct0_*.npz) on the prefix-only, few-shot and decoder-prompt branches, cached and
    use_cache=False; with num_return_sequences = 3 every group of three rows (item, draw) is the greedy row - the B * 3 decoder rows
    run over B encoder outputs with one cache and no reorder."""
    from test_t5_gpu import _model
    z, T, model, V = _model(tag, torch.float32)
    model.eval()
    fs = dict(prefix=T(z["fs_prefix"]), question_tokens=T(z["fs_tokens"]), question_mask=T(z["fs_mask"]), special_token_id=V - 1, max_length=9)
    dp = dict(prefix=T(z["fs_prefix"]), question_tokens=T(z["dp_tokens"]), question_mask=T(z["dp_mask"]), special_token_id=V - 1, max_length=9)
    branches = [
        (dict(prefix=T(z["prefix"]), max_length=9), z["gen_prefix_ids"]),
        (fs, z["gen_fs_ids"]),
        (dict(decoder_input_ids=T(z["dp_dec_a"]), decoder_attention_mask=torch.ones_like(T(z["dp_dec_a"])), **dp), z["gen_dp_a_ids"]),
        (dict(decoder_input_ids=T(z["dp_dec_b"]), decoder_attention_mask=T(z["dp_dec_b_mask"]), **dp), z["gen_dp_b_ids"]),
    ]
    for kw, want in branches:
        for use_cache in (True, False):
            for setting in (ONE_TOKEN if use_cache else ONE_TOKEN[:1]):
                got = model.generate(do_sample=True, seed=7, use_cache=use_cache, **setting, **kw)
                assert got.tolist() == want.tolist(), (setting, use_cache)
    for kw, want in branches[:2]:
        for use_cache in (True, False):
            got = model.generate(do_sample=True, top_k=1, num_return_sequences=3, use_cache=use_cache, **kw)
            assert got.shape[0] == 3 * want.shape[0]
            assert got.view(want.shape[0], 3, -1).tolist() == [[row] * 3 for row in want.tolist()], use_cache
    model.lm.native_step = False                                           # the same calls from Python (decode_step(beams=3))
    got = model.generate(do_sample=True, top_k=1, num_return_sequences=3, **fs)
    assert got.view(-1, 3, got.shape[1]).tolist() == [[row] * 3 for row in z["gen_fs_ids"].tolist()]


@pytest.mark.parametrize("name", ["hf_gpt2_tiny", "hf_opt_tiny"])
def test_causal_sampling_that_leaves_one_token_returns_the_greedy_ids(name):
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    path = os.path.join(GOLDEN, name)
    with open(os.path.join(path, "config.json")) as f:
        V = int(json.load(f)["vocab_size"])
    torch.manual_seed(3)
    L, D, B = 3, 16, 3
    model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version=path, dtype=torch.float32, device=DEV).eval()
    g = torch.Generator().manual_seed(5)
    special, n_img = V - 5, 2
    tok = torch.randint(3, special - n_img - 1, (B, 9), generator=g)
    mask = torch.ones(B, 9, dtype=torch.long)
    mask[1, -2:] = 0
    plain = dict(question_tokens=tok, prefix=torch.randn(B, D, generator=g), question_mask=mask, max_length=6, pad_token_id=0)
    tok_fs = tok.clone()
    for b in range(B):
        for i in range(n_img):
            tok_fs[b, 4 * i + (b % 2)] = special - i
    few = dict(question_tokens=tok_fs, prefix=torch.randn(B, n_img, D, generator=g), question_mask=mask, num_shots=n_img - 1,
               special_token_id=special, max_length=6, pad_token_id=0)
    for fn, kw in ((model.generate, plain), (model.generate_fewshot, few)):
        for use_cache in (True, False):
            want, want_lp = fn(use_cache=use_cache, output_scores=True, **kw)
            for setting in (ONE_TOKEN if use_cache else ONE_TOKEN[:1]):
                got, lp = fn(use_cache=use_cache, do_sample=True, seed=11, output_scores=True, **setting, **kw)
                assert got == want, (fn.__name__, setting, use_cache)
                assert lp.shape == want_lp.shape and (lp == 0).all()       # the log-probability under the processed distribution: log 1
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        model.generate(do_sample=True, num_return_sequences=2, **plain)
    free = [model.generate(do_sample=True, top_k=0, temperature=1.5, seed=s, **plain) for s in (1, 1, 2)]
    assert free[0] == free[1] and free[0] != free[2]


# ------------------------------------------------------------------------------------------------ 7. replay of a free run
def test_vct0_free_sampling_replays_from_its_scores_and_the_reference_philox():
    from test_t5_gpu import _model
    z, T, model, V = _model("t0", torch.float32)
    model.eval()
    kw = dict(prefix=T(z["fs_prefix"]), question_tokens=T(z["fs_tokens"]), question_mask=T(z["fs_mask"]), special_token_id=V - 1, max_length=9,
              do_sample=True, temperature=1.0, top_k=0, output_scores=True, return_dict_in_generate=True, num_return_sequences=2)
    seed = 424242
    out = model.generate(seed=seed, **kw)
    seq, scores = out.sequences, out.scores
    Rn = seq.shape[0]
    assert Rn == 2 * T(z["fs_tokens"]).shape[0] and len(scores) == seq.shape[1] - 1 and tuple(scores[0].shape) == (Rn, V)
    eos, pad = model.lm.cfg.eos_token_id, model.lm.cfg.pad_token_id
    pairs = skipped = 0
    for r in range(Rn):
        for j, sc in enumerate(scores):
            t = j + 1                                                      # decoder position = the step the kernel was given
            tok = int(seq[r, t])
            u = R.philox_uniform(seed, t, r)
            pairs += 1
            if R.cdf_margin(sc[r], u) < 1e-5:
                skipped += 1
            else:
                assert tok == R.inverse_cdf(sc[r], u), (r, t)
            assert math.isfinite(float(sc[r, tok]))
            if tok == eos:
                assert (seq[r, t + 1:] == pad).all()                       # finished rows emit pad afterwards
                break
    assert pairs >= Rn and skipped <= 0.02 * pairs, (skipped, pairs)
    again, other = model.generate(seed=seed, **kw), model.generate(seed=seed + 1, **kw)
    assert torch.equal(again.sequences, seq)
    assert other.sequences.shape != seq.shape or not torch.equal(other.sequences, seq)
    pairs_of_rows = seq.view(-1, 2, seq.shape[1])
    assert not torch.equal(pairs_of_rows[:, 0], pairs_of_rows[:, 1])       # the two draws of an item are different streams
    # seed=None: the seed comes from torch.initial_seed() and a per-model call counter that starts again with a new global seed
    runs = []
    for global_seed in (77, 78, 77):
        torch.manual_seed(global_seed)
        runs.append([model.generate(**kw).sequences for _ in range(2)])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
    assert not all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert runs[0][0].shape != runs[0][1].shape or not torch.equal(runs[0][0], runs[0][1])      # the second call draws another seed
