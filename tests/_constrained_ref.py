"""Plain-Python restatement of decoding inside a closed answer set (``eavqa_trie_constrain``), written from the definition (no trie, no
transformers): the generated ids are compared with every member of the set.  tests/test_constrained_cpu.py pins :func:`mask` to HF's
``PrefixConstrainedLogitsProcessor`` driven by :func:`allowed_fn`; the GPU tests compare the kernel with :func:`mask`."""
import torch


def walk(sequences, history, eos):
    """The ids allowed after the generated ids ``history`` (a list) for the set ``sequences`` (lists of ids, none holding ``eos``):
    the next id of every member that ``history`` is a strict prefix of, plus ``eos`` when ``history`` is a member; ``[eos]`` alone
    once ``history`` holds eos (the row has ended) or is no prefix of any member (it left the set).  Sorted, distinct."""
    h = [int(t) for t in history]
    n = len(h)
    out = set()
    for s in sequences:
        s = [int(t) for t in s]
        if len(s) >= n and s[:n] == h:
            out.add(s[n] if len(s) > n else int(eos))
    return sorted(out) if out else [int(eos)]


def item_sets(sequences, per_item, n_rows):
    """The set of every row: ``sequences`` for all, or ``per_item[row // rows_per_item]``."""
    if per_item is None:
        return [sequences] * n_rows
    assert n_rows % len(per_item) == 0
    rows = n_rows // len(per_item)
    return [per_item[r // rows] for r in range(n_rows)]


def mask(scores, history, prompt_len, cur_len, eos, sequences=None, per_item=None, to_logprobs=False):
    """The processed copy of float32 ``scores`` [R, V]: columns outside ``walk(...)`` of the row become -inf, the others keep their bits
    (``to_logprobs``: of ``log_softmax(scores)``)."""
    s = scores.clone().float()
    if to_logprobs:
        s = torch.log_softmax(s, dim=-1)
    out = torch.full_like(s, float("-inf"))
    sets = item_sets(sequences, per_item, s.shape[0])
    for r in range(s.shape[0]):
        allowed = walk(sets[r], history[r, prompt_len:cur_len].tolist() if cur_len > prompt_len else [], eos)
        out[r, allowed] = s[r, allowed]
    return out


def allowed_fn(eos, prompt_len, sequences=None, per_item=None, rows_per_item=1):
    """HF's ``prefix_allowed_tokens_fn(batch_id, input_ids)`` for the set(s).  HF calls it with ``batch_id`` = the item's index (rows are
    viewed as [-1, num_beams]); with several draws per item the rows are items to HF, hence ``rows_per_item``."""
    def fn(batch_id, input_ids):
        seqs = sequences if per_item is None else per_item[int(batch_id) // rows_per_item]
        return walk(seqs, input_ids[prompt_len:].tolist(), eos)
    return fn


def cut(row, eos, start=0):
    """A generated row's ids from ``start`` up to (not including) the first eos."""
    body = [int(t) for t in row[start:]]
    return body[:body.index(eos)] if eos in body else body
