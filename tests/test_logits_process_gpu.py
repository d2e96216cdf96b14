"""GPU: ``eavqa_logits_process`` against tests/_logits_ref.py (which tests/test_logits_ref_cpu.py pins to HF's processor classes), and
``eavqa_beam_step_logprobs`` behind it against ``eavqa_beam_step``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _logits_ref as ref

DEV = "cuda"
SENTINEL = 3.0e38                  # pad columns: a read would poison the row's log-sum-exp, a write shows
SHAPES = [(1, 7, 7), (3, 64, 64), (2, 1000, 1001), (2, 5000, 5000), (2, 32128, 32192)]       # 1001: the unaligned path; 5000: past 4096 columns
HISTORIES = [1, 5, 300, 1100]      # 1100 > the workgroup's 1024 threads: a second loop pass over the history


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


_CASES = {}


def case(R, V, ld, cur_len, scale):
    """Scores, history and bad words of one (shape, history) pair: built once, shared by the tests, never modified."""
    key = (R, V, ld, cur_len, scale)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * V + cur_len)
        s = torch.full((R, ld), SENTINEL)
        s[:, :V] = torch.randn(R, V, generator=g) * scale
        h = torch.randint(0, V, (R, cur_len), generator=g)
        if cur_len == 5:
            h[:, 2], h[:, 4] = h[:, 0], h[:, 1]                   # duplicates; the last token repeats an earlier one (a bigram match)
        if cur_len >= 300:
            h[:, -1] = h[:, 100]                                  # the suffix occurs earlier: n = 2 bans h[:, 101]
            h[:, -2] = h[:, 99]                                   # ... and n = 3 as well
        if scale > 2:                                             # (exact mode) a zero and a -inf on tokens the history holds
            s[0, int(h[0, 0])] = 0.0
            s[R - 1, int(h[R - 1, -1])] = -math.inf
        last = [int(t) for t in h[0, -2:]]
        words = [[int(V // 2)], [9 % V, 11 % V, 13 % V] if cur_len < 3 else last + [V - 1], [1 % V] * 9, last[-1:] + [int(V // 3)]]
        _CASES[key] = (s, h, words)
    return _CASES[key]


def run(ops, s, h, V, words=None, eos=None, **kw):
    x = s.clone().to(DEV)
    bw = bl = None
    if words:
        width = max(len(w) for w in words)
        bw = torch.zeros(len(words), width, dtype=torch.int32)
        for i, w in enumerate(words):
            bw[i, :len(w)] = torch.tensor(w, dtype=torch.int32)
        bw, bl = bw.to(DEV), torch.tensor([len(w) for w in words], dtype=torch.int32, device=DEV)
    ops.logits_process(x, V, h.to(DEV) if h is not None else None, 0 if h is None else h.shape[1], eos_token_id=eos, bad_words=bw, bad_lens=bl, **kw)
    torch.cuda.synchronize()
    return x.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


RULES = [dict(repetition_penalty=1.5), dict(repetition_penalty=0.5, no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2),
         dict(repetition_penalty=1.3, no_repeat_ngram_size=3, suppress_eos=True, bad=True), dict(bad=True)]


@pytest.mark.parametrize("cur_len", HISTORIES)
@pytest.mark.parametrize("R,V,ld", SHAPES)
def test_sparse_rules_are_the_reference_bit_for_bit(ops, R, V, ld, cur_len):
    s, h, words = case(R, V, ld, cur_len, 4.0)
    eos = V - 2 if V > 2 else 0
    for rules in RULES:
        rules = dict(rules)
        bad = words if rules.pop("bad", False) else None
        want = ref.process(s[:, :V], h, bad_words=bad, eos=eos, **rules)
        got = run(ops, s, h, V, words=bad, eos=eos, **rules)
        assert (got[:, V:] == SENTINEL).all(), rules                                       # pad columns keep their sentinel
        assert torch.equal(bits(got[:, :V]), bits(want)), rules                            # touched and untouched elements alike
        changed = bits(got[:, :V]) != bits(s[:, :V])
        touched = torch.zeros(R, V, dtype=torch.bool)
        touched.scatter_(1, h, True)
        for w in bad or []:
            touched[:, w[-1]] = True
        touched[:, eos] = True
        assert not (changed & ~touched).any(), rules                                       # nothing outside the history, the words and eos
        n = rules.get("no_repeat_ngram_size", 0)
        if n == 1:                                                                         # penalised AND banned reads -inf
            assert all((got[r, h[r]] == -math.inf).all() for r in range(R))
        if n in (2, 3) and cur_len >= 300:
            assert (got[torch.arange(R), h[:, 101]] == -math.inf).all()
        if rules.get("suppress_eos"):
            assert (got[:, eos] == -math.inf).all()
        if bad:
            assert (got[:, V // 2] == -math.inf).all()
            assert torch.equal(got[:, 1 % V] == -math.inf, want[:, 1 % V] == -math.inf)    # the 9-token word: only where the reference says


@pytest.mark.parametrize("R,V,ld", [(3, 64, 64), (2, 1000, 1001)])
def test_out_of_range_ids_and_an_inactive_call_change_nothing(ops, R, V, ld):
    s, h, _ = case(R, V, ld, 5, 4.0)
    far = h.clone()
    far[:, 0::2] += V                                                                       # >= V
    far[:, 1::2] -= V + 7                                                                   # < 0
    got = run(ops, s, far, V, words=[[V], [V + 5, 2 ** 31 - 1], [3, -1]], repetition_penalty=1.5, no_repeat_ngram_size=1)
    assert torch.equal(bits(got), bits(s))
    # out-of-range ids still MATCH like any id: the suffix (far, far') occurs earlier, so the in-range successor is banned
    mixed = far.clone()
    mixed[:, 2], mixed[:, 3], mixed[:, 4] = mixed[:, 0], 5, mixed[:, 0]
    want = ref.process(s[:, :V], mixed, no_repeat_ngram_size=2)
    got = run(ops, s, mixed, V, no_repeat_ngram_size=2)
    assert torch.equal(bits(got[:, :V]), bits(want)) and (got[:, 5] == -math.inf).all()
    assert torch.equal(bits(run(ops, s, h, V)), bits(s))                                    # no rule active
    assert torch.equal(bits(run(ops, s, None, V, no_repeat_ngram_size=2, repetition_penalty=1.2)), bits(s))      # an empty history


@pytest.mark.parametrize("to_logprobs", [False, True])
@pytest.mark.parametrize("R,V,ld", [(3, 64, 64), (2, 1000, 1001)])
def test_an_empty_history_bans_one_token_words_and_nothing_else(ops, R, V, ld, to_logprobs):
    """``cur_len = 0`` is the first step of the causal loop.  A one-token word bans at any history (HF: length-1 biases are unconditional);
    a longer word has no prefix to match yet.  The n-gram rule and the penalty have nothing to act on; the eos rule holds as always."""
    s, _, _ = case(R, V, ld, 5, 1.0 if to_logprobs else 4.0)
    eos = V - 2
    words = [[V // 2], [3, V - 1], [5], [7, 8, 9], [V + 4]]
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_eos=True)
    want = ref.process(s[:, :V], None, bad_words=words, eos=eos, to_logprobs=to_logprobs, float64_logprobs=to_logprobs, **rules)
    for h in (None, torch.zeros(R, 4, dtype=torch.int64)):                                  # no history at all, and one of which 0 ids count
        x = s.clone().to(DEV)
        bw = torch.zeros(len(words), 3, dtype=torch.int32)
        for i, w in enumerate(words):
            bw[i, :len(w)] = torch.tensor(w, dtype=torch.int32)
        ops.logits_process(x, V, None if h is None else h.to(DEV), 0, eos_token_id=eos, bad_words=bw.to(DEV),
                           bad_lens=torch.tensor([len(w) for w in words], dtype=torch.int32, device=DEV), to_logprobs=to_logprobs, **rules)
        got = x.cpu()
        assert (got[:, V:] == SENTINEL).all()
        banned = got[:, :V] == -math.inf
        assert torch.equal(banned, want == -math.inf)
        mine = s[:, :V] == -math.inf                                                        # (-inf on input stays -inf)
        mine[:, [V // 2, 5, eos]] = True
        assert torch.equal(banned, mine)                                                    # the two one-token words and eos, per row
        if to_logprobs:
            assert (got[:, :V].double()[~banned] - want[~banned]).abs().max().item() <= 1e-5
        else:
            assert torch.equal(bits(got[:, :V]), bits(want))


@pytest.mark.parametrize("cur_len", HISTORIES)
@pytest.mark.parametrize("R,V,ld", SHAPES)
def test_logprobs_mode_is_the_float64_log_softmax_then_the_rules(ops, R, V, ld, cur_len):
    """Within 1e-5 of float64: fp32 rounding of a sum over V terms and of two subtractions at magnitudes <= 16 (unit-variance scores,
    log V <= 10.4) stays an order of magnitude below; a penalty of 1.3 scales value and error alike."""
    s, h, words = case(R, V, ld, cur_len, 1.0)
    eos = V - 2 if V > 2 else 0
    for rules in (dict(), dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_eos=True, bad=True)):
        rules = dict(rules)
        bad = words if rules.pop("bad", False) else None
        want = ref.process(s[:, :V], h, bad_words=bad, eos=eos, to_logprobs=True, float64_logprobs=True, **rules)
        got = run(ops, s, h, V, words=bad, eos=eos, to_logprobs=True, **rules)
        assert (got[:, V:] == SENTINEL).all()
        assert torch.equal(got[:, :V] == -math.inf, want == -math.inf), rules
        keep = want != -math.inf
        err = (got[:, :V].double()[keep] - want[keep]).abs().max().item() if keep.any() else 0.0
        print(f"[{R}x{V} ld {ld} cur_len {cur_len} {sorted(rules)}] max |logprob diff| {err:.2e}")
        assert err <= 1e-5, rules


@pytest.mark.parametrize("V,pad", [(50, False), (96, True), (32128, True)])
def test_no_rule_logprobs_path_is_beam_step(ops, V, pad):
    """``logits_process(to_logprobs=1)`` with no rule + ``beam_step(logprobs=True)`` = ``beam_step``: tokens and parents exact, running
    scores within 1e-5, over the six-step scenario of tests/test_beam_gpu.py (ranking gaps >= 1e-3, asserted there and here)."""
    from test_beam_gpu import MARGIN, MAX_LENGTH, SEEDS, _scenario
    B, k, lp, es = 3, 3, 2.0, False
    ld = (V + 32 + 3) // 4 * 4 if pad else V
    steps, gap = _scenario(SEEDS.get((k, V), 0), B, k, V, ld, lp, es)
    assert gap >= MARGIN, gap
    a, b = ops.BeamState(B, k, MAX_LENGTH, 0, 1, DEV), ops.BeamState(B, k, MAX_LENGTH, 0, 1, DEV)
    for step, s in enumerate(steps, start=1):
        for st in (a, b):
            st.improve.copy_(s["before"]["improve"].to(torch.int32))
        ops.beam_step(s["logits"].to(DEV), V, a, step, s["eos"], lp, es)
        lg = s["logits"].to(DEV)
        ops.logits_process(lg, V, b.run_seq, step, to_logprobs=True)
        assert (lg[:, V:] == s["logits"][0, V:].to(DEV)).all()
        ops.beam_step(lg, V, b, step, s["eos"], lp, es, logprobs=True)
        what = f"step {step}"
        assert torch.equal(a.next_tokens, b.next_tokens) and torch.equal(a.parents, b.parents), what
        assert torch.equal(a.run_seq, b.run_seq) and torch.equal(a.pool_seq, b.pool_seq) and torch.equal(a.pool_fin, b.pool_fin), what
        assert torch.equal(a.cont, b.cont), what
        real = a.run_scores > -1.0e8
        assert torch.equal(real, b.run_scores > -1.0e8), what
        if real.any():                                             # (after the last step every running score carries the -1e9 sentinel)
            assert (a.run_scores[real] - b.run_scores[real]).abs().max().item() <= 1e-5, what


def test_minus_inf_log_probabilities_rank_last(ops):
    """``eavqa_beam_step_logprobs`` on rows where all but 2k - 1 entries are -inf: the finite ones are chosen in order, never a pad column."""
    B, k, V, ld = 1, 2, 40, 44
    lg = torch.full((B * k, ld), SENTINEL)
    lg[:, :V] = -math.inf
    lg[0, [3, 17, 30]] = torch.tensor([-0.5, -1.5, -2.5])
    lg[1, [5, 6, 7]] = torch.tensor([-0.25, -1.25, -2.25])
    st = ops.BeamState(B, k, 6, 0, 1, DEV)
    st.run_scores.copy_(torch.tensor([[0.0, -0.125]]))
    ops.beam_step(lg.to(DEV), V, st, 1, 39, 1.0, False, logprobs=True)
    assert st.next_tokens.tolist() == [5, 3] and st.parents.tolist() == [1, 0]
    assert torch.equal(st.run_scores.cpu(), torch.tensor([[-0.375, -0.5]]))
