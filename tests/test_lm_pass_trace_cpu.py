"""CPU: the entry-point calls of the full-sequence Python passes are pinned.

``FrozenCausalLM.forward`` / ``backward``, ``decode.score_decode``, ``FrozenT5.forward_train`` / ``backward`` / ``score`` and the
transformer mapper are pure enqueue, so what they do is the list of ``eavqa_*`` calls they make.  tests/_lm_pass_trace.py records that
list on CPU tensors (real library, recording ``call``) for the cases of tests/_lm_pass_cases.py; tests/golden/lm_pass_trace.txt is that
output recorded before the passes were restated as one causal layer loop per route with named tapes; the Llama cases and the cached
generation route (``decode._prefill`` / ``_decode_step``: the ``*_cached`` cases) were recorded before the Llama family was folded into
that loop and the block driver chosen once per cache.  A later native driver of the training pass is held to the same lines."""
import os
import re

import pytest

import _lm_pass_trace as tracer

GOLDEN = os.path.join(tracer.ROOT, "tests", "golden", "lm_pass_trace.txt")


@pytest.fixture(scope="module")
def trace():
    from eavqa_amd import build
    build.build()
    return tracer.trace_all()


def test_call_sequences_equal_the_recording(trace):
    with open(GOLDEN) as f:
        golden = "".join(line for line in f if not line.startswith("#"))
    got, want = tracer.parse(trace), tracer.parse(golden)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
    assert trace == golden


def test_every_lookahead_region_is_the_b_operand_of_the_next_gemm(trace):
    """What the hand-written hint chains are meant to be: a non-null look-ahead region of an ``eavqa_gemm_pf`` call is the whole B operand
    of the next GEMM-family call of the case.  The one hint without a successor is the lm_head named behind the last layer of a pass that
    returns hidden rows (``logits="none"``): the head GEMM is then the caller's."""
    hints = 0
    for name, calls in tracer.parse(trace).items():
        gemms = [c.split() for c in calls if c.split()[0] in tracer.GEMM_FAMILY]
        for cur, nxt in zip(gemms, gemms[1:] + [None]):
            if cur[0] != "eavqa_gemm_pf" or cur[-2] == "0":
                continue
            hints += 1
            if nxt is None:
                head = "head+0" if name.startswith("llama_") else "wte+0"                 # (the tiny GPT-2 / OPT tie the head to wte, the tiny Llama does not)
                assert "logits_none" in name and cur[-2] == head, (name, cur)
                continue
            b = nxt[1 + tracer.GEMM_FAMILY[nxt[0]]]
            n, k = (int(nxt[5]), int(nxt[6])) if nxt[0] != "eavqa_gemm_splitk" else (int(nxt[3]), int(nxt[4]))
            assert cur[-2] == b and int(cur[-1]) == n * k * 2, (name, cur, nxt)
    assert hints > 100


def test_the_cases_cover_every_route(trace):
    cases = tracer.parse(trace)
    assert len(cases) == 69 and all(cases.values())
    called = lambda name, entry: sum(c.startswith(entry + " ") for c in cases[name])
    assert called("gpt2_bf16_train_fold", "eavqa_gemm_ln") and not called("gpt2_bf16_hidden_fold", "eavqa_gemm_pf")   # (the backward hints)
    assert not called("gpt2_bf16_train_no_prefetch", "eavqa_gemm_pf") and called("gpt2_bf16_train_packed_scored", "eavqa_gemm_pf")
    assert called("fp8_train_fused_quantizer", "eavqa_layernorm_fwd_fp8") and not called("fp8_train_separate_quantizer", "eavqa_layernorm_fwd_fp8")
    assert called("opt_fp32_score_shared", "eavqa_attention_merge") == 2 and not called("opt_fp32_score_shared", "eavqa_gemm_pf")
    assert not called("opt_fp32_score_replicated", "eavqa_attention_merge")
    assert called("llama_bf16_train_packed", "eavqa_rope") == 4 and called("llama_bf16_train_packed", "eavqa_swiglu_bwd")
    assert not called("llama_bf16_train_no_prefetch", "eavqa_gemm_pf") and called("llama_bf16_train_packed_scored", "eavqa_gemm_pf")
    blocks = ("eavqa_lm_block_forward", "eavqa_lm_block_forward_fp8", "eavqa_llama_block_forward")
    cached = [name for name in cases if name.endswith("_cached")]
    assert len(cached) == 7
    for name in cached:                                       # prefill + two steps, each one call of the family's own block driver
        own = "eavqa_llama_block_forward" if name.startswith("llama_") else "eavqa_lm_block_forward_fp8" if name.startswith("fp8_") else blocks[0]
        assert [called(name, b) for b in blocks] == [3 * (b == own) for b in blocks], name
    assert all(re.match(r"eavqa_\w+ ", c) for calls in cases.values() for c in calls)
