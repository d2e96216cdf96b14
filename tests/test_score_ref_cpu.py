"""CPU: tests/_score_ref.py (the float64 restatement the GPU scoring tests compare against) pinned to transformers.  Nothing is
downloaded: a tiny T5 built from a config, and the committed tiny GPT-2 / OPT directories."""
import os

import numpy as np
import pytest
import torch

import _score_ref as ref
from conftest import GOLDEN


def _candidates(V, C, Tc, seed):
    """[C, Tc] int64 right-padded with -100: 1 .. Tc - 1 content tokens in [3, V - 4) plus a closing token."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.full((C, Tc), ref.PAD, dtype=torch.int64)
    for c in range(C):
        n = int(torch.randint(1, Tc, (1,), generator=g))
        cand[c, :n] = torch.randint(3, V - 4, (n,), generator=g)
        cand[c, n] = 1
    return cand


def test_t5_loss_times_tokens_is_the_restated_sum():
    from transformers import T5Config, T5ForConditionalGeneration
    torch.manual_seed(0)
    cfg = T5Config(vocab_size=96, d_model=32, d_kv=8, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=4, feed_forward_proj="gated-gelu",
                   tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    model = T5ForConditionalGeneration(cfg).eval()
    ids = torch.randint(3, 90, (1, 7), generator=torch.Generator().manual_seed(1))
    cand = _candidates(96, 5, 4, seed=2)
    with torch.no_grad():
        for c in range(cand.shape[0]):
            lab = cand[c:c + 1]
            out = model(input_ids=ids, labels=lab)
            n = int((lab != ref.PAD).sum())
            lp = ref.token_logprobs(out.logits.double().numpy(), lab.numpy())
            score, cnt, _ = ref.candidate_scores(lp[None], lab.numpy()[None])
            assert int(cnt[0, 0]) == n
            assert abs(-float(out.loss) * n - float(score[0, 0])) <= 1e-5 * n


@pytest.mark.parametrize("name", ["hf_gpt2_tiny", "hf_opt_tiny"])
def test_causal_loss_times_tokens_is_the_restated_sum(name):
    from transformers import AutoModelForCausalLM
    model = AutoModelForCausalLM.from_pretrained(os.path.join(GOLDEN, name)).eval().float()
    V = model.config.vocab_size
    prompt = torch.randint(3, V - 4, (1, 6), generator=torch.Generator().manual_seed(3))
    cand = _candidates(V, 5, 4, seed=4)
    with torch.no_grad():
        for c in range(cand.shape[0]):
            n = int((cand[c] != ref.PAD).sum())
            seq = torch.cat([prompt, cand[c:c + 1, :n]], dim=1)
            lab = torch.cat([torch.full_like(prompt, ref.PAD), cand[c:c + 1, :n]], dim=1)
            out = model(input_ids=seq, labels=lab)
            # HF shifts inside the loss: position p predicts token p + 1; the restatement gathers at the candidate's own positions
            rows = out.logits[0, prompt.shape[1] - 1:prompt.shape[1] - 1 + n].double().numpy()
            lp = ref.token_logprobs(rows, cand[c, :n].numpy())
            score, cnt, _ = ref.candidate_scores(lp[None, None], cand[c, :n].numpy()[None, None])
            assert int(cnt[0, 0]) == n
            assert abs(-float(out.loss) * n - float(score[0, 0])) <= 1e-5 * n


def test_ignored_ids_length_penalty_and_the_stable_order():
    lp = np.log(np.array([[[0.5, 0.25, 0.5], [0.5, 0.25, 0.5], [0.125, 0.5, 0.5], [0.5, 0.5, 0.5]]]))
    lab = np.array([[[5, 1, -100], [5, 1, -100], [7, 8, 1], [2, 1, -100]]])
    s, n, masked = ref.candidate_scores(lp, lab)
    assert n.tolist() == [[2, 2, 3, 2]] and masked[0, 0, 2] == 0.0
    assert np.allclose(s[0], np.log([0.125, 0.125, 0.125 * 0.25, 0.25]))
    assert ref.stable_order(s).tolist() == [[3, 0, 1, 2]]                      # the exact tie keeps the smaller index first
    s1, n1, _ = ref.candidate_scores(lp, lab, ignored_ids=(0, 1, 2), length_penalty=1.0)
    assert n1.tolist() == [[1, 1, 2, 0]] and np.isneginf(s1[0, 3])              # nothing scored: -inf
    assert np.allclose(s1[0, :3], [np.log(0.5), np.log(0.5), np.log(0.125 * 0.5) / 2])
    assert ref.stable_order(np.array([[np.nan, -np.inf, 1.0, -np.inf, 2.0]])).tolist() == [[4, 2, 1, 3, 0]]
    f32, _, _ = ref.candidate_scores(lp, lab, length_penalty=0.5, dtype=np.float32)
    assert f32.dtype == np.float32 and np.allclose(f32, s / np.sqrt(n), rtol=1e-6)


def test_merge_of_two_segments_is_attention_over_the_concatenated_keys():
    rng = np.random.default_rng(0)
    Q, K1, K2, d = 6, 11, 4, 16
    q, k1, v1 = rng.standard_normal((Q, d)), rng.standard_normal((K1, d)), rng.standard_normal((K1, d))
    k2, v2 = rng.standard_normal((K2, d)), rng.standard_normal((K2, d))
    vis1 = np.ones((Q, K1), dtype=bool)
    vis1[:, 3] = vis1[:, 7] = False
    vis1[2] = False                                                             # a query that sees no key of the first segment
    vis2 = np.tril(np.ones((Q, K2), dtype=bool), k=K2 - Q + 2)
    vis2[:, 0] = True
    o1, l1 = ref.softmax_segment(q, k1, v1, vis1, 0.25)
    o2, l2 = ref.softmax_segment(q, k2, v2, vis2, 0.25)
    assert np.isneginf(l1[2])
    want, _ = ref.softmax_segment(q, np.concatenate([k1, k2]), np.concatenate([v1, v2]), np.concatenate([vis1, vis2], axis=1), 0.25)
    got = ref.lse_merge(o1, l1, o2, l2)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[2], o2[2])                                        # bit for bit the second segment's row
    assert np.isfinite(got).all()
