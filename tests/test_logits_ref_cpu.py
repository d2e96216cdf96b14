"""CPU: tests/_logits_ref.py (the restatement the GPU tests compare ``eavqa_logits_process`` with) equals HF's own processor classes,
applied in ``_get_logits_processor`` order, bit for bit on seeded cases - raw logits and the beam variant on ``log_softmax``."""
import math

import pytest
import torch

import _logits_ref as ref
from transformers.generation.logits_process import (LogitsProcessorList, MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
                                                    NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor)

V, EOS = 23, 5


def hf(scores, history, rp=1.0, n=0, bad=None, min_length=0, min_new_tokens=0, prompt_len=1):
    procs = LogitsProcessorList()
    if rp != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=rp))
    if n > 0:
        procs.append(NoRepeatNGramLogitsProcessor(n))
    if bad:
        procs.append(NoBadWordsLogitsProcessor(bad, EOS))
    if min_length > 0:
        procs.append(MinLengthLogitsProcessor(min_length, EOS))
    if min_new_tokens > 0:
        procs.append(MinNewTokensLengthLogitsProcessor(prompt_len, min_new_tokens, EOS))
    return procs(history, scores.clone())


def mine(scores, history, rp=1.0, n=0, bad=None, min_length=0, min_new_tokens=0, prompt_len=1, **kw):
    return ref.process(scores, history, repetition_penalty=rp, no_repeat_ngram_size=n, bad_words=bad, eos=EOS,
                       suppress_eos=ref.suppress_eos(history.shape[1], prompt_len, min_length, min_new_tokens), **kw)


def same(a, b):
    """Bit for bit; -0.0 and +0.0 count as equal (HF's bad-word bias is an addition of 0.0, which turns a -0.0 into +0.0)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all()) and torch.equal(a.isinf(), b.isinf())


def scores_and_history(seed, R=4, cur_len=6):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(R, V, generator=g) * 3
    s[0, 2], s[1, 3], s[2, 7] = 0.0, -math.inf, 0.0             # scores of exactly 0 and of -inf, on tokens the histories hold
    h = torch.randint(0, V, (R, cur_len), generator=g)
    if cur_len >= 4:
        h[0, :4] = torch.tensor([2, 9, 2, 9])                    # duplicates; the bigram (2, 9) twice
        h[1, -2:] = torch.tensor([3, 3])
        h[2, 0], h[2, -1] = 7, 7
    return s, h


HISTORIES = [1, 2, 3, 6]
RULES = [dict(rp=0.5), dict(rp=1.5), dict(n=1), dict(n=2), dict(n=3), dict(min_length=4), dict(min_length=2), dict(min_new_tokens=3),
         dict(min_new_tokens=3, prompt_len=3), dict(rp=1.5, n=2, min_new_tokens=4), dict(rp=0.5, n=1, min_length=9)]


@pytest.mark.parametrize("cur_len", HISTORIES)
@pytest.mark.parametrize("rules", RULES, ids=[",".join(f"{k}={v}" for k, v in r.items()) for r in RULES])
@pytest.mark.parametrize("logprobs", [False, True])
def test_restatement_equals_hf(rules, cur_len, logprobs):
    """Includes n > cur_len (n = 3 at cur_len 1, 2), n == cur_len, duplicates, zero and -inf scores, both penalty directions."""
    s, h = scores_and_history(10 * cur_len + 1, cur_len=cur_len)
    want = hf(torch.log_softmax(s, -1) if logprobs else s, h, **rules)
    got = mine(s, h, to_logprobs=logprobs, **rules)
    assert same(got, want)
    if not logprobs and set(rules) == {"rp"} and cur_len == 6:
        # a duplicate history token is penalised once, a score of exactly 0 stays 0, -inf stays -inf
        assert got[0, 9] == (s[0, 9] * rules["rp"] if s[0, 9] < 0 else s[0, 9] / rules["rp"]) and got[0, 2] == 0.0 and got[1, 3] == -math.inf


BAD = [
    [[4]],                                   # single token
    [[2, 9, 11]],                            # multi-token: row 0's history ends (.., 2, 9) when cur_len == 4
    [[1, 2, 3, 4, 5, 6, 7, 8]],              # longer than the history
    [[9, 12], [2, 9, 12]],                   # two words ending in one token
    [[EOS], [4]],                            # [eos] is dropped
    [[4], [4]],                              # the same word twice
]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
@pytest.mark.parametrize("cur_len", [1, 4, 6])
def test_bad_words_equal_hf(bad, cur_len):
    s, h = scores_and_history(7 + cur_len, cur_len=cur_len)
    if cur_len == 4:
        h[3] = torch.tensor([1, 2, 2, 9])
    want = hf(s, h, bad=bad)
    got = mine(s, h, bad=bad)
    assert same(got, want)
    if bad == [[EOS], [4]]:
        assert torch.equal(got[:, EOS], s[:, EOS]) and (got[:, 4] == -math.inf).all()
    if bad == [[2, 9, 11]] and cur_len == 4:
        assert got[0, 11] == -math.inf and got[3, 11] == -math.inf and got[1, 11] == s[1, 11]
    if bad == [[1, 2, 3, 4, 5, 6, 7, 8]]:
        assert torch.equal(got, s)
    # together with every other rule, in HF's order
    assert same(mine(s, h, rp=1.3, n=2, bad=bad, min_length=5), hf(s, h, rp=1.3, n=2, bad=bad, min_length=5))


def test_a_penalised_and_banned_token_is_banned_and_out_of_range_ids_change_nothing():
    s, h = scores_and_history(3)
    got = mine(s, h, rp=1.5, n=1)
    for r in range(s.shape[0]):
        assert (got[r, h[r]] == -math.inf).all()
    far = torch.full_like(h, V + 100)
    assert torch.equal(mine(s, far, rp=1.5, n=1, bad=[[V + 3]]), s)
    assert torch.equal(mine(s, h[:, :0]), s)                    # an empty history and no rule


def test_float64_logprobs_variant_is_log_softmax_in_float64():
    s, h = scores_and_history(5)
    got = mine(s, h, n=2, to_logprobs=True, float64_logprobs=True)
    want = mine(s, h, n=2, to_logprobs=True)
    assert got.dtype == torch.float64 and torch.equal(got.isinf(), want.isinf())
    keep = ~want.isinf()
    assert (got[keep] - want[keep].double()).abs().max() <= 1e-5
