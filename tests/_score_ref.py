"""float64 restatement of answer-candidate scoring (what ``score_candidates`` and the kernels of csrc/score.hip compute): token
log-probabilities from logits, masked / ignored / length-normalised sums, the stable descending order, and the merge of two attention
segments by their log-sum-exps.  numpy only; tests/test_score_ref_cpu.py pins it to transformers."""
import numpy as np

PAD = -100


def token_logprobs(logits, labels):
    """``logits`` [..., V], ``labels`` int [...] (one label per row) or [..., n] (n labels per row): log_softmax(logits)[label] in
    float64; 0 where the label is outside [0, V)."""
    x = np.asarray(logits, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    V = x.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=-1, keepdims=True)
        lse = np.log(np.exp(x - m).sum(axis=-1, keepdims=True))
        lp = (x - m) - lse
    ok = (lab >= 0) & (lab < V)
    idx = np.where(ok, lab, 0)
    picked = np.take_along_axis(lp, idx, axis=-1) if lab.ndim == x.ndim else np.take_along_axis(lp, idx[..., None], axis=-1)[..., 0]
    return np.where(ok, picked, 0.0)


def scored_mask(labels, ignored_ids=()):
    lab = np.asarray(labels, dtype=np.int64)
    keep = lab >= 0
    for i in ignored_ids:
        keep &= lab != int(i)
    return keep


def candidate_scores(tok_logp, labels, ignored_ids=(), length_penalty=0.0, dtype=np.float64):
    """``tok_logp`` / ``labels`` [B, C, T] -> (scores [B, C], n_tokens int32 [B, C], masked tok_logp).  The sum runs over t in index
    order in ``dtype`` (float32 restates the kernel's arithmetic bit for bit: exponents 0, 1 and 0.5 divide by 1, n and sqrt(n))."""
    lp = np.asarray(tok_logp, dtype=dtype)
    keep = scored_mask(labels, ignored_ids)
    lp = np.where(keep, lp, dtype(0))
    B, C, T = lp.shape
    total = np.zeros((B, C), dtype=dtype)
    for t in range(T):
        total = np.where(keep[..., t], (total + lp[..., t]).astype(dtype), total)
    n = keep.sum(axis=-1).astype(np.int32)
    nf = n.astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        if length_penalty == 0.0:
            scores = total
        elif length_penalty == 1.0:
            scores = (total / nf).astype(dtype)
        elif length_penalty == 0.5:
            scores = (total / np.sqrt(nf).astype(dtype)).astype(dtype)
        else:
            scores = (total / np.power(nf, dtype(length_penalty)).astype(dtype)).astype(dtype)
    scores = np.where(n == 0, dtype(-np.inf), scores)
    return scores, n, lp


def stable_order(scores):
    """Per row: indices by descending score, equal scores with the smaller index first; -inf behind every number, NaN behind -inf."""
    s = np.asarray(scores)
    out = np.empty(s.shape, dtype=np.int32)
    for b in range(s.shape[0]):
        cls = np.where(np.isnan(s[b]), 2, np.where(np.isneginf(s[b]), 1, 0))
        key = np.where(cls == 0, -s[b].astype(np.float64), 0.0)
        out[b] = np.lexsort((np.arange(s.shape[1]), key, cls))
    return out


def min_rank_gap(scores):
    """Smallest difference between scores adjacent in the ranking, over all rows."""
    s = -np.sort(-np.asarray(scores, dtype=np.float64), axis=1)
    return float((s[:, :-1] - s[:, 1:]).min()) if s.shape[1] > 1 else float("inf")


def softmax_segment(q, k, v, visible, scale=1.0):
    """One attention segment in float64: ``q`` [Q, d], ``k`` / ``v`` [K, d], ``visible`` bool [Q, K].  Returns (out [Q, d], lse [Q]);
    a row without a visible key reports lse = -inf and an output of zeros."""
    s = (np.asarray(q, np.float64) @ np.asarray(k, np.float64).T) * scale
    s = np.where(visible, s, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s.max(axis=1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        p = np.exp(s - m)
        l = p.sum(axis=1, keepdims=True)
        out = np.where(l > 0, (p @ np.asarray(v, np.float64)) / np.where(l > 0, l, 1.0), 0.0)
        lse = np.where(l[:, 0] > 0, m[:, 0] + np.log(l[:, 0]), -np.inf)
    return out, lse


def lse_merge(o1, l1, o2, l2):
    """Attention over the union of two key sets from the segments' outputs [Q, d] and log-sum-exps [Q].  A segment with lse = -inf has
    weight 0: the other segment's output passes through unchanged (both empty: the second's)."""
    o1, o2 = np.asarray(o1, np.float64), np.asarray(o2, np.float64)
    l1, l2 = np.asarray(l1, np.float64), np.asarray(l2, np.float64)
    e1, e2 = np.isneginf(l1), np.isneginf(l2)
    m = np.maximum(np.where(e1, l2, l1), np.where(e2, l1, l2))
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(invalid="ignore"):
        w1 = np.where(e1, 0.0, np.exp(l1 - m))
        w2 = np.where(e2, 0.0, np.exp(l2 - m))
    den = w1 + w2
    mixed = (w1[:, None] * o1 + w2[:, None] * o2) / np.where(den > 0, den, 1.0)[:, None]
    return np.where(e1[:, None], o2, np.where(e2[:, None], o1, mixed))
