"""fp32 torch restatement of the logits processors ``eavqa_logits_process`` implements, written rule by rule from their definitions (not
by calling transformers): tests/test_logits_ref_cpu.py pins it to HF's own processor classes, the GPU tests compare the kernel with it.

Order (HF ``GenerationMixin._get_logits_processor``, transformers 5.15): repetition penalty -> no-repeat n-gram -> bad words ->
min length / min new tokens.  ``process`` works on a copy; ``to_logprobs`` first replaces every row by ``log_softmax`` (what HF's beam
search hands to its processors)."""
import math

import torch


def drop_eos_words(bad_words, eos):
    """HF ``NoBadWordsLogitsProcessor.__init__``: words equal to ``[eos]`` are dropped."""
    return [list(w) for w in (bad_words or []) if eos is None or list(w) != [eos]]


def process(scores, history, *, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words=None, eos=None, suppress_eos=False,
            to_logprobs=False, float64_logprobs=False):
    """``scores`` float32 [R, V] -> processed copy.  ``history`` int64 [R, cur_len] (cur_len may be 0).  Ids outside [0, V) change
    nothing.  ``float64_logprobs``: the log_softmax is taken in float64 and the result kept in float64 (the yardstick of the beam mode)."""
    R, V = scores.shape
    cur_len = history.shape[1] if history is not None else 0
    out = scores.clone()
    if to_logprobs:
        out = torch.log_softmax(out.double(), dim=-1) if float64_logprobs else torch.log_softmax(out, dim=-1)
    p = out.new_tensor(repetition_penalty)
    n = int(no_repeat_ngram_size)
    for r in range(R):
        h = [int(t) for t in history[r, :cur_len]] if cur_len else []
        if repetition_penalty != 1.0:
            for tok in dict.fromkeys(h):                                   # every distinct token once
                if 0 <= tok < V:
                    s = out[r, tok]
                    out[r, tok] = s * p if s < 0 else s / p
        banned = set()
        if n > 0 and cur_len >= n:
            suffix = h[cur_len - n + 1:]
            for i in range(cur_len - n + 1):
                if h[i:i + n - 1] == suffix:
                    banned.add(h[i + n - 1])
        for w in drop_eos_words(bad_words, eos):
            L = len(w)
            if L <= cur_len or L == 1:
                if L == 1 or h[cur_len - (L - 1):] == w[:-1]:
                    banned.add(w[-1])
        if suppress_eos:
            banned.add(int(eos))
        for tok in banned:
            if 0 <= tok < V:
                out[r, tok] = -math.inf
    return out


def suppress_eos(cur_len, prompt_len, min_length=0, min_new_tokens=0):
    """HF ``MinLengthLogitsProcessor`` / ``MinNewTokensLengthLogitsProcessor``: is eos held back at a history of ``cur_len`` ids."""
    return cur_len < min_length or (min_new_tokens > 0 and cur_len - prompt_len < min_new_tokens)
