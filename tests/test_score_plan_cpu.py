"""CPU: the host side of answer-candidate scoring - candidate validation, the chunk plan of the lm_head stage, the keyword contract of the
three ``score_candidates`` entry points, and ``eavqa_token_logprobs`` / ``eavqa_candidate_rank`` / ``eavqa_attention_merge`` returning
their error codes before any launch."""
import inspect

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ candidates
def test_candidates_are_checked_on_the_host():
    from eavqa_amd.models.scoring import prepare_candidates
    ok = torch.tensor([[[5, 6, -100], [7, -100, -100]], [[8, 9, 4], [3, 1, -100]]])
    assert torch.equal(prepare_candidates(ok, 2, "cpu"), ok)
    with pytest.raises(ValueError, match="without a token"):
        prepare_candidates(torch.tensor([[[5, 6], [-100, -100]]]), 1, "cpu")
    with pytest.raises(ValueError, match="C >= 1"):
        prepare_candidates(torch.empty((2, 0, 3), dtype=torch.int64), 2, "cpu")
    with pytest.raises(ValueError, match="C >= 1"):
        prepare_candidates(torch.empty((0, 3), dtype=torch.int64), 2, "cpu")
    with pytest.raises(ValueError, match="right-padded"):
        prepare_candidates(torch.tensor([[[5, -100, 6]]]), 1, "cpu")
    with pytest.raises(ValueError, match="-100"):
        prepare_candidates(torch.tensor([[[5, -1, -1]]]), 1, "cpu")
    with pytest.raises(ValueError, match="B = 3"):
        prepare_candidates(ok, 3, "cpu")
    with pytest.raises(ValueError):
        prepare_candidates(None, 2, "cpu")
    with pytest.raises(ValueError, match="integer"):
        prepare_candidates(torch.zeros(2, 2), 1, "cpu")


def test_a_shared_answer_list_is_broadcast_over_the_questions():
    from eavqa_amd.models.scoring import prepare_candidates
    shared = [[5, 6, 1], [7, 1, -100]]
    got = prepare_candidates(shared, 3, "cpu")
    assert got.shape == (3, 2, 3) and got.dtype == torch.int64 and got.is_contiguous()
    for b in range(3):
        assert got[b].tolist() == shared
    assert prepare_candidates(np.asarray(shared, dtype=np.int32), 1, "cpu").dtype == torch.int64


# ------------------------------------------------------------------------------------------------ chunk plan
@pytest.mark.parametrize("C,rows,vpad", [(1, 1, 64), (5, 12, 96), (64, 128, 32128), (1024, 96, 50304), (1024, 8, 128)])
def test_chunks_cover_the_candidates_within_the_byte_bound(C, rows, vpad):
    from eavqa_amd.models.scoring import LOGITS_BYTES_MAX, plan_chunks
    assert LOGITS_BYTES_MAX == 256 << 20
    chunks = plan_chunks(C, rows, vpad)
    assert chunks[0][0] == 0 and chunks[-1][1] == C
    for (a0, a1), (b0, _) in zip(chunks, chunks[1:]):
        assert a1 == b0
    for c0, c1 in chunks:
        assert c1 > c0 and (c1 - c0) * rows * vpad * 4 <= LOGITS_BYTES_MAX
    # as few buffers as the bound allows
    assert len(chunks) == -(-C // min(C, LOGITS_BYTES_MAX // (rows * vpad * 4)))


def test_chunks_of_one_candidate_are_legal_and_one_oversized_candidate_is_not():
    from eavqa_amd.models.scoring import plan_chunks
    assert plan_chunks(4, 12, 96, chunk=1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert plan_chunks(5, 12, 96, chunk=2) == [(0, 2), (2, 4), (4, 5)]
    assert plan_chunks(5, 12, 96, chunk=99) == [(0, 5)]
    assert plan_chunks(3, 2, 4, limit=2 * 4 * 4 * 2) == [(0, 2), (2, 3)]
    with pytest.raises(ValueError, match="exceed"):
        plan_chunks(3, 2, 4, limit=31)
    with pytest.raises(ValueError):
        plan_chunks(3, 2, 4, chunk=0)
    with pytest.raises(ValueError):
        plan_chunks(0, 2, 4)


# ------------------------------------------------------------------------------------------------ keywords
def test_entry_points_take_no_generation_keyword():
    from eavqa_amd.models.clipcap import ClipCaptionModel
    from eavqa_amd.models.scoring import reject_unknown
    from eavqa_amd.models.vct0 import VCT0Model
    reject_unknown("score_candidates", {})
    with pytest.raises(TypeError, match="num_beams"):
        reject_unknown("score_candidates", dict(num_beams=2))
    for fn, names in ((VCT0Model.score_candidates, ("prefix", "question_tokens", "question_mask", "candidates", "no_prefix",
                                                    "pass_examples_through_encoder_one_at_a_time", "num_shots", "special_token_id",
                                                    "length_penalty", "ignored_ids", "share_prompt")),
                      (ClipCaptionModel.score_candidates, ("question_tokens", "prefix", "question_mask", "candidates", "length_penalty",
                                                           "ignored_ids", "share_prompt")),
                      (ClipCaptionModel.score_candidates_fewshot, ("question_tokens", "prefix", "question_mask", "candidates", "num_shots",
                                                                   "special_token_id", "length_penalty", "ignored_ids", "share_prompt"))):
        sig = inspect.signature(fn)
        named = [p.name for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD and p.name != "self"]
        assert tuple(named) == names
        assert sig.parameters["length_penalty"].default == 0.0 and sig.parameters["share_prompt"].default is True
        assert sig.parameters["ignored_ids"].default == ()
    # the keyword check comes first: nothing of the model is touched before it
    for fn in (VCT0Model.score_candidates, ClipCaptionModel.score_candidates, ClipCaptionModel.score_candidates_fewshot):
        for bad in ("do_sample", "num_beams", "repetition_penalty", "max_length"):
            with pytest.raises(TypeError, match=bad):
                fn(None, None, None, candidates=[[1]], **{bad: 1})


# ------------------------------------------------------------------------------------------------ rank_from_ensembles (host contract)
def test_rank_from_ensembles_needs_a_member():
    from eavqa_amd.utils.ensembling import rank_from_ensembles
    with pytest.raises(ValueError):
        rank_from_ensembles(lambda i: None, 0)


def test_ensemble_sum_and_rank_restated_in_numpy():
    """What ``rank_from_ensembles`` computes, restated: float32 sums in member order, then the stable descending order (the device run of
    the function itself is in tests/test_score_kernels_gpu.py)."""
    import _score_ref as ref
    rng = np.random.default_rng(1)
    members = [rng.standard_normal((3, 6)).astype(np.float32) for _ in range(3)]
    members[1][0, 2] = -np.inf
    members[0][1, 4] = members[0][1, 1]
    members[1][1, 4] = members[1][1, 1]
    members[2][1, 4] = members[2][1, 1]                                           # an exact tie after the sum
    total = members[0].copy()
    for m in members[1:]:
        total = (total + m).astype(np.float32)
    order = ref.stable_order(total)
    assert order[0, -1] == 2
    row = order[1].tolist()
    assert row.index(1) + 1 == row.index(4)
    assert np.array_equal(np.take_along_axis(total, order.astype(np.int64), 1)[2], -np.sort(-total[2]))


# ------------------------------------------------------------------------------------------------ the entry points, before any launch
P = 4096      # a non-null, 16-byte aligned value standing in for a device pointer: every call below must return before it is used


def test_token_logprobs_rejects_bad_arguments_before_any_launch(lib):
    def call(R=2, V=32, logits=P, ld=32, labels=P, ld_labels=4, n=4, out=P, ld_out=4):
        return lib.eavqa_token_logprobs(R, V, logits, ld, labels, ld_labels, n, out, ld_out, None)

    assert call(logits=None) == -1 and call(labels=None) == -1 and call(out=None) == -1
    assert call(R=0) == -1 and call(V=0) == -1 and call(n=0) == -1 and call(R=-3) == -1
    assert call(V=33) == -3 and call(ld_labels=3) == -3 and call(ld_out=3) == -3
    assert call(n=65, ld_labels=65, ld_out=65) == -3


def test_candidate_rank_rejects_bad_arguments_before_any_launch(lib):
    def call(B=2, C=3, T=4, ptrs=None, ign=None, n_ign=0, lp=0.0):
        ptrs = [P] * 5 if ptrs is None else ptrs
        return lib.eavqa_candidate_rank(B, C, T, ptrs[0], ptrs[1], ign, n_ign, lp, ptrs[2], ptrs[3], ptrs[4], None)

    for i in range(5):
        assert call(ptrs=[None if j == i else P for j in range(5)]) == -1
    assert call(B=0) == -1 and call(C=0) == -1 and call(T=0) == -1
    assert call(n_ign=-1) == -1 and call(n_ign=2) == -1 and call(lp=float("nan")) == -1      # ids announced but not given
    assert call(C=1025) == -3 and call(ign=P, n_ign=17) == -3


def test_attention_merge_rejects_bad_arguments_before_any_launch(lib):
    def call(dtype=0, B=2, C=3, T=5, H=3, hd=16, ptrs=None, ld=(48, 48, 48)):
        ptrs = [P] * 5 if ptrs is None else ptrs
        return lib.eavqa_attention_merge(dtype, B, C, T, H, hd, ptrs[0], ld[0], ptrs[1], ptrs[2], ld[1], ptrs[3], ptrs[4], ld[2], None)

    for i in range(5):
        assert call(ptrs=[None if j == i else P for j in range(5)]) == -1
    assert call(dtype=2) == -1 and call(dtype=-1) == -1
    assert call(B=0) == -1 and call(C=0) == -1 and call(T=0) == -1 and call(H=0) == -1 and call(hd=0) == -1
    assert call(hd=18, ld=(56, 56, 56)) == -3                                     # fp32: hd % 4
    assert call(dtype=1, hd=20, ld=(64, 64, 64)) == -3                            # bf16: hd % 8
    assert call(ld=(47, 48, 48)) == -3 and call(ld=(48, 44, 48)) == -3 and call(ld=(48, 48, 40)) == -3       # narrower than H * hd
    assert call(ld=(50, 48, 48)) == -3 and call(dtype=1, ld=(52, 48, 48)) == -3   # rows off the 16-byte grid
    assert call(ptrs=[P + 4, P, P, P, P]) == -2 and call(ptrs=[P, P, P + 8, P, P]) == -2 and call(ptrs=[P, P, P, P, P + 2]) == -2
