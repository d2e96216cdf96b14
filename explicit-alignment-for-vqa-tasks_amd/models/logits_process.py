"""The logits-processor arguments of HF ``generate`` (``repetition_penalty``, ``no_repeat_ngram_size``, ``min_length``,
``min_new_tokens``, ``bad_words_ids``), checked on the host once for the encoder-decoder (``VCT0Model.generate``) and the causal
(``ClipCaptionModel.generate`` / ``generate_fewshot``) path.

The rules themselves are ``eavqa_logits_process`` (one kernel per step, in place on the step's scores, in the order of HF's
``_get_logits_processor``: repetition penalty -> n-gram -> bad words -> min length -> min new tokens; temperature / top-k / top-p follow
inside ``eavqa_sample_pick``).  With no rule active there is no plan, and then no launch and no allocation."""
from __future__ import annotations

import math
import numbers
import operator
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

LOGITS_KWARGS = ("repetition_penalty", "no_repeat_ngram_size", "min_length", "min_new_tokens", "bad_words_ids")
MAX_BAD_WORDS = 1024              # the limits of eavqa_logits_process
MAX_BAD_WORD_LENGTH = 16
MAX_HISTORY = 2048                # ids per row the kernel stages; a history never passes max_length


@dataclass(frozen=True)
class LogitsPlan:
    """What ``eavqa_logits_process`` needs besides the scores and the history.  ``repetition_penalty`` 1.0 = off, the sizes 0 = off,
    ``bad_words`` () = off (``[eos]`` entries already dropped, as HF's ``NoBadWordsLogitsProcessor`` does)."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_length: int = 0
    min_new_tokens: int = 0
    bad_words: Tuple[Tuple[int, ...], ...] = ()
    eos_token_id: Optional[int] = None

    def suppress_eos(self, cur_len: int, prompt_len: int) -> bool:
        """HF ``MinLengthLogitsProcessor`` / ``MinNewTokensLengthLogitsProcessor`` at a history of ``cur_len`` ids."""
        return cur_len < self.min_length or (self.min_new_tokens > 0 and cur_len - prompt_len < self.min_new_tokens)

    def upload(self, V: int, device) -> "DeviceLogitsPlan":
        return DeviceLogitsPlan(self, V, device)


class DeviceLogitsPlan:
    """A :class:`LogitsPlan` with its bad-word table on the device: built ONCE per ``generate`` call, never per step."""

    def __init__(self, plan: LogitsPlan, V: int, device):
        self.plan = plan
        self.bad_words = self.bad_lens = None
        self.n_bad = self.bad_width = 0
        if plan.bad_words:
            over = sorted({t for w in plan.bad_words for t in w if t >= V})
            if over:
                raise ValueError(f"bad_words_ids: the vocabulary holds {V} tokens, but {over} were named (HF raises likewise)")
            self.n_bad, self.bad_width = len(plan.bad_words), max(len(w) for w in plan.bad_words)
            table = torch.zeros((self.n_bad, self.bad_width), dtype=torch.int32)
            for i, w in enumerate(plan.bad_words):
                table[i, :len(w)] = torch.tensor(w, dtype=torch.int32)
            self.bad_words = table.to(device)
            self.bad_lens = torch.tensor([len(w) for w in plan.bad_words], dtype=torch.int32).to(device)

    def apply(self, scores, V: int, history, cur_len: int, prompt_len: int, to_logprobs: bool = False) -> None:
        """The rules for the step that follows a history of ``cur_len`` ids, in place on ``scores`` float32 [R, >= V]."""
        from .. import ops
        p = self.plan
        ops.logits_process(scores, V, history, cur_len, repetition_penalty=p.repetition_penalty, no_repeat_ngram_size=p.no_repeat_ngram_size,
                           eos_token_id=p.eos_token_id, suppress_eos=p.suppress_eos(cur_len, prompt_len), bad_words=self.bad_words,
                           bad_lens=self.bad_lens, to_logprobs=to_logprobs)


def _index(v) -> Optional[int]:
    """``v`` as an int if it is an integer (Python's or numpy's, as HF accepts; not a bool, not a float), else None."""
    if isinstance(v, bool) or type(v).__name__ in ("bool_", "bool"):          # numpy's bool still answers __index__
        return None
    try:
        return operator.index(v)
    except TypeError:
        return None


def _int_arg(kw: dict, name: str) -> int:
    v = kw.get(name)
    if v is None:
        return 0
    i = _index(v)
    if i is None or i < 0:
        raise ValueError(f"{name}={v!r}: an integer >= 0 (0 or None = off)")
    return i


def processing_plan(kw: dict) -> Optional[LogitsPlan]:
    """``kw``: generation arguments by name (missing or None = off), plus ``eos_token_id`` (one id or None) and ``max_length`` (None = not
    checked) as the path resolved them.  None when no rule is active."""
    eos, max_length = kw.get("eos_token_id"), kw.get("max_length")
    rp = kw.get("repetition_penalty")
    if rp is None:
        rp = 1.0
    elif isinstance(rp, bool) or not isinstance(rp, numbers.Real) or not (rp > 0 and math.isfinite(rp)):
        raise ValueError(f"repetition_penalty={rp!r}: a finite float > 0 (1.0 or None = off; HF raises likewise)")
    rp = float(rp)
    n = _int_arg(kw, "no_repeat_ngram_size")
    ml, mnt = _int_arg(kw, "min_length"), _int_arg(kw, "min_new_tokens")
    if kw.get("min_length") is not None and kw.get("min_new_tokens") is not None:
        raise ValueError("min_length together with min_new_tokens: HF lets min_new_tokens replace min_length with a warning; pass one of them")
    for name, v in (("min_length", ml), ("min_new_tokens", mnt)):
        if v and max_length is not None and v > max_length:
            raise ValueError(f"{name}={v} is larger than max_length={max_length} (HF raises likewise)")
        if v and eos is None:
            raise ValueError(f"{name}={v} without an eos_token_id: there is no token to hold back (HF would silently drop the processor)")
    words = kw.get("bad_words_ids")
    bad: Tuple[Tuple[int, ...], ...] = ()
    if words is not None:
        if not isinstance(words, (list, tuple)) or len(words) == 0:
            raise ValueError(f"bad_words_ids={words!r}: a non-empty list of non-empty lists of token ids (HF raises likewise)")
        for w in words:
            if not isinstance(w, (list, tuple)) or len(w) == 0 or any(_index(t) is None or _index(t) < 0 for t in w):
                raise ValueError(f"bad_words_ids={words!r}: every word is a non-empty list of integers >= 0 (HF raises likewise)")
        if len(words) > MAX_BAD_WORDS or max(len(w) for w in words) > MAX_BAD_WORD_LENGTH:
            raise NotImplementedError(f"bad_words_ids: at most {MAX_BAD_WORDS} words of at most {MAX_BAD_WORD_LENGTH} tokens each are built")
        bad = tuple(dict.fromkeys(w for w in (tuple(_index(t) for t in w) for w in words) if eos is None or w != (int(eos),)))
    if rp == 1.0 and n == 0 and ml == 0 and mnt == 0 and not bad:
        return None
    if max_length is not None and max_length > MAX_HISTORY:
        raise NotImplementedError(f"max_length={max_length} with a logits processor: eavqa_logits_process holds a history of at most "
                                  f"{MAX_HISTORY} ids")
    return LogitsPlan(rp, n, ml, mnt, bad, None if eos is None else int(eos))


def split_logits_kwargs(kw: dict) -> Tuple[dict, dict]:
    """``kw`` without the processor arguments, and those (for a path whose other checks reject names they do not know)."""
    return {k: v for k, v in kw.items() if k not in LOGITS_KWARGS}, {k: v for k, v in kw.items() if k in LOGITS_KWARGS}
