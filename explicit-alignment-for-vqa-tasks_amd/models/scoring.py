"""Answer-candidate scoring (rank classification): the host side both LM families share.

``score_candidates`` answers "which of these C answers does the frozen LM prefer, and by how much": per question the log-probability of
every candidate token given the prompt (images, shots, question), the per-candidate sums and the ranking.  The prompt is encoded (T5) or
prefilled (causal LM) once per question; the two model paths live in ``FrozenT5.score`` (models/t5.py) and ``score_decode``
(models/decode.py).  Here: argument checks, the chunk plan of the lm_head stage, that stage itself, and the result object.

The lm_head stage runs ONE head GEMM per candidate (the B * Tq hidden rows of candidate c, gathered into a contiguous block) into a
logits buffer that holds a chunk of candidates, then one ``eavqa_token_logprobs`` over the chunk.  The GEMM of a candidate has the same
shape whatever the chunk size is, so chunking changes where a row of logits lives and nothing else: every result bit is the same for any
chunk size.  No logits buffer exceeds ``LOGITS_BYTES_MAX``.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

from .. import ops

Tensor = torch.Tensor

LOGITS_BYTES_MAX = 256 << 20
CHUNK_CANDIDATES: Optional[int] = None       # tests: force the chunk size (candidates per logits buffer); None = as many as the bound allows
PAD_LABEL = -100


class CandidateScores:
    """Result of ``score_candidates``; every tensor is on the device.  ``scores`` float32 [B, C]; ``token_logprobs`` float32 [B, C, Tc]
    (0 at pads and ignored ids); ``n_tokens`` int32 [B, C] (scored tokens); ``order`` int32 [B, C] (candidates by descending score, equal
    scores with the smaller index first); ``best`` = ``order[:, 0]``."""

    def __init__(self, scores: Tensor, token_logprobs: Tensor, n_tokens: Tensor, order: Tensor):
        self.scores, self.token_logprobs, self.n_tokens, self.order = scores, token_logprobs, n_tokens, order

    @property
    def best(self) -> Tensor:
        return self.order[:, 0]


def reject_unknown(name: str, kwargs: dict) -> None:
    """``score_candidates`` takes no sampling, beam or processor keyword: an unknown keyword is a TypeError naming it, as Python's own."""
    if kwargs:
        raise TypeError(f"{name}() got an unexpected keyword argument {sorted(kwargs)[0]!r}")


def prepare_candidates(candidates, B: int, device) -> Tensor:
    """int64 [B, C, Tc] on ``device`` from [B, C, Tc] or a [C, Tc] list shared by all questions, right-padded with -100.  Checked on the
    host: C >= 1, every candidate holds a token, the padding is on the right."""
    if candidates is None:
        raise ValueError("score_candidates needs `candidates`")
    cand = torch.as_tensor(candidates)
    if cand.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"candidates must be integer token ids (got {cand.dtype})")
    if cand.dim() == 2:
        cand = cand.unsqueeze(0).expand(B, -1, -1)
    if cand.dim() != 3 or cand.shape[0] != B:
        raise ValueError(f"candidates must be [B, C, Tc] with B = {B}, or [C, Tc] (got {tuple(cand.shape)})")
    if cand.shape[1] < 1 or cand.shape[2] < 1:
        raise ValueError("score_candidates needs at least one candidate (C >= 1) of at least one token")
    host = cand.detach().to("cpu", torch.int64)
    real = host >= 0
    if not bool(real[..., 0].all()):
        raise ValueError("a candidate without a token cannot be scored")
    if bool((host[~real] != PAD_LABEL).any()):
        raise ValueError("candidates are padded with -100; other negative ids are not token ids")
    if bool((real[..., 1:] & ~real[..., :-1]).any()):
        raise ValueError("candidates must be right-padded: a token follows a pad")
    return host.to(device).contiguous()


def plan_chunks(C: int, rows_per_candidate: int, vpad: int, chunk: Optional[int] = None, limit: int = LOGITS_BYTES_MAX) -> List[Tuple[int, int]]:
    """Candidate ranges [(c0, c1), ...] covering 0 .. C such that a float32 logits buffer of (c1 - c0) * rows_per_candidate rows of
    ``vpad`` columns stays within ``limit`` bytes.  ``chunk`` caps the candidates per range (1 is legal)."""
    if C < 1 or rows_per_candidate < 1 or vpad < 1:
        raise ValueError("plan_chunks: C, rows_per_candidate and vpad must be positive")
    per = rows_per_candidate * vpad * 4
    if per > limit:
        raise ValueError(f"the logits of one candidate ({per} bytes for {rows_per_candidate} rows) exceed the {limit}-byte bound: score fewer questions per call")
    n = limit // per
    if chunk is not None:
        if chunk < 1:
            raise ValueError("plan_chunks: chunk must be >= 1")
        n = min(n, int(chunk))
    n = min(n, C)
    return [(c0, min(c0 + n, C)) for c0 in range(0, C, n)]


def score_hidden(hidden: Tensor, idx: Tensor, labels: Tensor, head: Callable[[Tensor, Tensor], None], V: int, vpad: int) -> Tensor:
    """The lm_head stage.  ``hidden`` [N, E] final hidden rows; ``idx`` int32 [C, B * Tq]: the rows of candidate c ordered (b, t);
    ``labels`` int64 [B, C, Tq]; ``head(h, out)`` writes the logits of rows ``h`` into float32 ``out`` [rows, V].  Returns float32
    [B, C, Tq] token log-probabilities (0 at labels < 0)."""
    B, C, Tq = labels.shape
    n = B * Tq
    tok = torch.empty((B, C, Tq), device=hidden.device, dtype=torch.float32)
    for c0, c1 in plan_chunks(C, n, vpad, CHUNK_CANDIDATES):
        lg = torch.empty(((c1 - c0) * n, vpad), device=hidden.device, dtype=torch.float32)
        for c in range(c0, c1):
            head(ops.gather_rows(hidden, idx[c]), lg[(c - c0) * n:(c - c0 + 1) * n, :V])
        lab = labels[:, c0:c1].permute(1, 0, 2).reshape(-1, 1).contiguous()          # rows (c, b, t), as the buffer
        lp = ops.token_logprobs(lg, V, lab)
        tok[:, c0:c1] = lp.view(c1 - c0, B, Tq).permute(1, 0, 2)
    return tok


def finish(tok_logp: Tensor, labels: Tensor, ignored_ids: Sequence[int], length_penalty: float) -> CandidateScores:
    """Sums, counts and the ranking (``eavqa_candidate_rank``) over float32 ``tok_logp`` / int64 ``labels`` [B, C, Tc]."""
    if labels.shape[1] > 1024:
        raise ValueError("score_candidates ranks at most 1024 candidates per question")
    tok_logp = tok_logp.contiguous()
    scores, n_tokens, order = ops.candidate_rank(tok_logp, labels.contiguous(), tuple(int(i) for i in ignored_ids), float(length_penalty))
    return CandidateScores(scores, tok_logp, n_tokens, order)
