"""GPU: the three kernels of csrc/score.hip against tests/_score_ref.py - ``eavqa_token_logprobs`` (also bit-equal to gathering from
``eavqa_logits_process(to_logprobs=1)``), ``eavqa_candidate_rank`` (bit-equal sums, exact order) and ``eavqa_attention_merge`` (against
ONE ``eavqa_attention_fwd`` call over the concatenated keys) - and ``rank_from_ensembles`` on the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _score_ref as ref

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ eavqa_token_logprobs
@pytest.mark.parametrize("n_labels", [1, 5, 64])
@pytest.mark.parametrize("V,pad", [(50, 0), (50, 14), (96, 0), (96, 32), (32128, 0), (32128, 64)])
def test_token_logprobs_match_float64_and_the_logits_processor_bit_for_bit(ops, V, pad, n_labels):
    R, ld = 7, V + pad
    g = torch.Generator().manual_seed(V + pad + n_labels)
    buf = torch.full((R, ld), float("nan"))                                   # a pad column that is read turns the row into NaN
    buf[:, :V] = torch.randn(R, V, generator=g) * 3.0
    buf[3, 1:V:3] = float("-inf")
    labels = torch.randint(0, V, (R, n_labels), generator=g)
    labels[0, 0], labels[1, -1], labels[2, 0] = -100, 0, V - 1
    if n_labels >= 5:
        labels[4, 1], labels[4, 2], labels[4, 3] = -100, V - 1, 0
        labels[3, 2] = 1                                                      # a -inf entry of the -inf row
    logits = buf.to(DEV)
    got = ops.token_logprobs(logits[:, :V], V, labels.to(DEV))
    want = ref.token_logprobs(buf[:, :V].numpy(), labels.numpy())
    got_h = got.cpu().numpy()
    finite = np.isfinite(want)
    assert np.array_equal(np.isneginf(want), np.isneginf(got_h)) and not np.isnan(got_h).any()
    assert np.abs(got_h[finite] - want[finite]).max() <= 1e-5
    assert (got_h[labels.numpy() < 0] == 0).all()
    # the same bits as the processor's log_softmax of a copy, gathered
    copy = logits.clone()
    ops.logits_process(copy, V, None, 0, to_logprobs=True)
    gathered = torch.where(labels.to(DEV) >= 0, copy[:, :V].gather(1, labels.clamp_min(0).to(DEV)), torch.zeros((), device=DEV))
    assert torch.equal(got, gathered)
    assert torch.equal(logits[:, :V], buf[:, :V].to(DEV))                     # the logits themselves are only read


def test_token_logprobs_label_beyond_the_vocabulary_writes_zero(ops):
    V = 50
    logits = torch.randn(2, 64, generator=torch.Generator().manual_seed(0)).to(DEV)
    labels = torch.tensor([[3, V, 10 ** 12], [V - 1, 49, 50]], dtype=torch.int64, device=DEV)
    got = ops.token_logprobs(logits, V, labels).cpu()
    assert got[0, 1] == 0 and got[0, 2] == 0 and got[1, 2] == 0 and got[0, 0] < 0 and got[1, 0] == got[1, 1]


# ------------------------------------------------------------------------------------------------ eavqa_candidate_rank
def _rank_case(B, C, T, seed):
    g = torch.Generator().manual_seed(seed)
    lp = -torch.rand(B, C, T, generator=g) * 6.0
    labels = torch.randint(0, 12, (B, C, T), generator=g)
    lens = torch.randint(1, T + 1, (B, C), generator=g)
    labels = torch.where(torch.arange(T)[None, None, :] < lens[..., None], labels, torch.full_like(labels, -100))
    if C >= 5:
        src, dst = (3, 700) if C > 700 else (0, 3)
        lp[:, dst], labels[:, dst] = lp[:, src], labels[:, src]                # an exact tie
        labels[0, 1, 0], lp[0, 1, 0] = 7, float("-inf")                        # a -inf score
        labels[0, 2] = torch.tensor([1, 2, 0][:T] + [-100] * max(0, T - 3))   # nothing left once (0, 1, 2) are ignored
    return lp, labels


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("ignored", [(), (0, 1, 2)])
@pytest.mark.parametrize("B,C,T", [(1, 1, 1), (3, 5, 4), (2, 1024, 3)])
def test_candidate_rank_sums_bit_equal_and_order_exact(ops, B, C, T, ignored, length_penalty):
    lp, labels = _rank_case(B, C, T, seed=B * 1000 + C + T)
    dev_lp = lp.to(DEV).contiguous()
    scores, n_tokens, order = ops.candidate_rank(dev_lp, labels.to(DEV).contiguous(), ignored, length_penalty)
    want, want_n, want_lp = ref.candidate_scores(lp.numpy(), labels.numpy(), ignored, length_penalty, dtype=np.float32)
    got = scores.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(n_tokens.cpu().numpy(), want_n) and n_tokens.dtype == torch.int32
    assert np.array_equal(order.cpu().numpy(), ref.stable_order(want)) and order.dtype == torch.int32
    assert np.array_equal(dev_lp.cpu().numpy(), want_lp)                       # entries that are not scored were zeroed in place
    if C >= 5:
        row = order[0].tolist()
        a, b = (3, 700) if C > 700 else (0, 3)
        assert row.index(a) + 1 == row.index(b)                               # the tie: the smaller index first, adjacent
        assert np.isneginf(got[0, 1]) and all(np.isneginf(got[0, c]) for c in row[row.index(1):])      # -inf ranks behind every number


def test_candidate_rank_orders_minus_infinity_and_nan_last(ops):
    s = torch.tensor([[[float("nan")], [float("-inf")], [1.0], [float("-inf")], [2.0], [float("inf")]]])
    scores, n, order = ops.candidate_rank(s.to(DEV), torch.zeros(s.shape, dtype=torch.int64, device=DEV))
    assert order.tolist() == [[5, 4, 2, 1, 3, 0]]
    assert order.tolist() == ref.stable_order(s[..., 0].numpy()).tolist()


def test_rank_from_ensembles_sums_the_members_and_ranks_once(ops):
    from eavqa_amd.models.scoring import CandidateScores
    from eavqa_amd.utils.ensembling import rank_from_ensembles
    rng = np.random.default_rng(1)
    B, C, T, n = 3, 6, 2, 3
    toks = [rng.standard_normal((B, C, T)).astype(np.float32) for _ in range(n)]
    toks[1][0, 2, 0] = -np.inf
    for t in toks:
        t[1, 4] = t[1, 1]                                                      # an exact tie after the sum
    members = []
    for t in toks:
        s = (t[..., 0] + t[..., 1]).astype(np.float32)
        members.append(CandidateScores(torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV), torch.full((B, C), T, dtype=torch.int32, device=DEV),
                                       torch.zeros((B, C), dtype=torch.int32, device=DEV)))
    out = rank_from_ensembles(lambda i: members[i], n)
    total = members[0].scores.cpu().numpy().copy()
    for m in members[1:]:
        total = (total + m.scores.cpu().numpy()).astype(np.float32)
    assert np.array_equal(out.scores.cpu().numpy().view(np.int32), total.view(np.int32))
    assert np.array_equal(out.order.cpu().numpy(), ref.stable_order(total))
    assert torch.equal(out.best, out.order[:, 0]) and out.order[0, -1].item() == 2
    assert np.allclose(out.token_logprobs.cpu().numpy()[np.isfinite(toks[1])], sum(toks)[np.isfinite(toks[1])], atol=1e-6)
    assert torch.equal(members[0].scores.cpu(), torch.from_numpy((toks[0][..., 0] + toks[0][..., 1]).astype(np.float32)))     # inputs untouched


# ------------------------------------------------------------------------------------------------ eavqa_attention_merge
def _merge_case(ops, dtype, hd, mask_all_of_row=None):
    B, C, T, H, S0 = 2, 3, 5, 3, 11
    E = H * hd
    g = torch.Generator().manual_seed(hd)
    mk = lambda rows: torch.randn(rows, E, generator=g).to(dtype).to(DEV)
    q, kp, vp, kc, vc = mk(B * C * T), mk(B * S0), mk(B * S0), mk(B * C * T), mk(B * C * T)
    mask = torch.ones(B, S0, dtype=torch.int32)
    mask[1, 2] = mask[1, 9] = 0                                                # two masked prompt keys in one row
    if mask_all_of_row is not None:
        mask[mask_all_of_row] = 0
    mask = mask.to(DEV)
    scale = hd ** -0.5
    o1, l1 = ops.attention_fwd(q, kp, vp, B, H, C * T, S0, hd, key_mask=mask, causal=False, scale=scale, save_lse=True)
    o2, l2 = ops.attention_fwd(q, kc, vc, B * C, H, T, T, hd, causal=True, scale=scale, save_lse=True)
    # the replicated problem: every candidate sees [its question's prompt | its own tokens] in ONE softmax
    kcat = torch.cat([kp.view(B, 1, S0, E).expand(B, C, S0, E), kc.view(B, C, T, E)], dim=2).reshape(B * C * (S0 + T), E).contiguous()
    vcat = torch.cat([vp.view(B, 1, S0, E).expand(B, C, S0, E), vc.view(B, C, T, E)], dim=2).reshape(B * C * (S0 + T), E).contiguous()
    mcat = torch.cat([mask.repeat_interleave(C, dim=0), torch.ones(B * C, T, dtype=torch.int32, device=DEV)], dim=1).contiguous()
    want = ops.attention_fwd(q, kcat, vcat, B * C, H, T, S0 + T, hd, key_mask=mcat, causal=True, scale=scale)
    return (B, C, T, H), (o1, l1, o2, l2), want


@pytest.mark.parametrize("hd", [16, 64, 80])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_merge_of_prompt_and_candidate_segments_is_one_attention_over_all_keys(ops, dtype, hd):
    (B, C, T, H), (o1, l1, o2, l2), want = _merge_case(ops, dtype, hd)
    keep = o2.clone()
    got = ops.attention_merge(o1, l1, o2, l2, B, C, T, H, hd, out=torch.empty_like(o2))
    err = (got.double() - want.double()).abs().max().item()
    # fp32: 1e-5.  bf16: two segment roundings, the final rounding and the single call's own rounding, each <= 2^-9 relative
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7 * want.float().abs().max().item()
    print(f"[{dtype} hd={hd}] merge vs one call over the concatenated keys: max |diff| {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    assert torch.equal(o2, keep)
    inplace = ops.attention_merge(o1, l1, o2, l2, B, C, T, H, hd)                # out = o2
    assert inplace.data_ptr() == o2.data_ptr() and torch.equal(inplace, got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_merge_passes_the_second_segment_through_when_the_first_saw_no_key(ops, dtype):
    hd = 64
    (B, C, T, H), (o1, l1, o2, l2), want = _merge_case(ops, dtype, hd, mask_all_of_row=1)
    got = ops.attention_merge(o1, l1, o2, l2, B, C, T, H, hd, out=torch.empty_like(o2))
    rows = C * T
    assert torch.equal(got[rows:], o2[rows:])                                  # question 1: bit for bit the candidate segment
    assert not torch.equal(got[:rows], o2[:rows]) and torch.isfinite(got.float()).all()
    assert (l1[1] < -0.25 * torch.finfo(torch.float32).max).all() and (l1[0] > -1e30).all()
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7 * want.float().abs().max().item()
    assert (got[:rows].double() - want[:rows].double()).abs().max().item() <= tol


# ------------------------------------------------------------------------------------------------ batches beyond one launch grid
@pytest.mark.parametrize("dtype,hd,rel", [(torch.float32, 16, False), (torch.bfloat16, 64, False), (torch.bfloat16, 64, True)])
def test_attention_forward_splits_a_batch_beyond_the_grid_limit(ops, dtype, hd, rel):
    """B * H > 65 535 (questions x candidates as batch entries): the wrapper launches over consecutive samples; outputs and log-sum-exps
    equal two calls on the halves bit for bit, with a key mask, a batch stride on the keys and T5's bias table."""
    B, H, Sq, Sk, rows_k = 2100, 32, 3, 5, 7
    assert B * H > ops.ATTN_MAX_PAIRS
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B * Sq, H * hd, generator=g).to(dtype).to(DEV)
    k, v = (torch.randn(B * rows_k, H * hd, generator=g).to(dtype).to(DEV) for _ in range(2))
    mask = (torch.rand(B, Sk, generator=g) > 0.3).int()
    mask[:, 0] = 1
    mask = mask.to(DEV)
    table = torch.randn(H, 2 * Sk - 1, generator=g).to(DEV) if rel else None
    kw = dict(key_mask=mask, causal=True, scale=hd ** -0.5, save_lse=True, kv_batch_rows=rows_k)

    def run(b0, b1):
        args = (q[b0 * Sq:b1 * Sq], k[b0 * rows_k:b1 * rows_k], v[b0 * rows_k:b1 * rows_k], b1 - b0, H, Sq, Sk, hd)
        if rel:
            return ops.attention_fwd_rel(*args, rel_bias=table, rel_zero=Sk - 1, key_mask=mask[b0:b1], **{n: x for n, x in kw.items() if n != "key_mask"})
        return ops.attention_fwd(*args, **{**kw, "key_mask": mask[b0:b1]})

    o, lse = run(0, B)
    half = B // 2
    (o1, l1), (o2, l2) = run(0, half), run(half, B)
    assert torch.equal(o, torch.cat([o1, o2])) and torch.equal(lse, torch.cat([l1, l2]))
    assert torch.isfinite(o.float()).all()
