"""Host plan of an interleaved image-text training row (``insert_prefix_into_input`` src/models/vct0.py:494-533 with labels).

Pure torch on whatever device the inputs live on; nothing here loads the HIP library, so the module imports without a GPU.  The
device side of the same layout is ``eavqa_build_fewshot_rows`` (tokens, mask, positions; through ``ops.build_fewshot_labels`` also the labels).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

Tensor = torch.Tensor

SENTINEL_ERROR = "every row must hold exactly one sentinel token per image"


class InterleavePlan(NamedTuple):
    """``lengths``: attended positions per expanded row (host ints) and ``label_count``: labels != -100 at non-sentinel positions
    (host int) - both None when the inputs live on the device, where the forward counts for itself; ``T_out`` = T + (L-1)*n_img."""
    lengths: Optional[List[int]]
    label_count: Optional[int]
    T_out: int


def is_sentinel(tokens: Tensor, n_img: int, special_token_id: int) -> Tensor:
    """A token is a sentinel iff special - n_img < tok <= special (the test of ``fewshot_rows_kernel``)."""
    return (tokens <= special_token_id) & (tokens > special_token_id - n_img)


def check_sentinels(status: Tensor, n_img: int) -> None:
    """``status``: sentinels found per row (host count, or what ``eavqa_build_fewshot_rows`` wrote): one read."""
    if not bool((status == n_img).all().item()):
        raise ValueError(SENTINEL_ERROR)           # the reference's .view at vct0.py:512 fails


def interleave_plan(question_tokens: Tensor, question_mask: Optional[Tensor], labels: Optional[Tensor], L: int, n_img: int,
                    special_token_id: int) -> InterleavePlan:
    """Row lengths and label count of the expanded rows.  A sentinel counts whatever its mask says (its L slots are always attended,
    as in ``fewshot_rows_kernel``); a label on a sentinel is never scored.  With host tensors everything is computed here and the
    sentinel count is validated; with device tensors ``lengths`` / ``label_count`` are None and the caller validates the kernel's
    ``status`` with :func:`check_sentinels`."""
    if question_tokens.dim() != 2:
        raise ValueError("question_tokens must be [B, T]")
    B, T = question_tokens.shape
    if L <= 0 or n_img <= 0:
        raise ValueError("L and n_img must be positive")
    for name, t in (("question_mask", question_mask), ("labels", labels)):
        if t is not None and tuple(t.shape) != (B, T):
            raise ValueError(f"{name} must be [B, T] = {(B, T)} like question_tokens, got {tuple(t.shape)}")
    T_out = T + (L - 1) * n_img
    host = all(t is None or not t.is_cuda for t in (question_tokens, question_mask, labels))
    if not host:
        return InterleavePlan(None, None, T_out)
    sent = is_sentinel(question_tokens, n_img, special_token_id)
    check_sentinels(sent.sum(1), n_img)
    attended = ~sent if question_mask is None else (~sent & (question_mask != 0))
    lengths = [int(n) + L * n_img for n in attended.sum(1).tolist()]
    count = int(((labels != -100) & ~sent).sum()) if labels is not None else None
    return InterleavePlan(lengths, count, T_out)
