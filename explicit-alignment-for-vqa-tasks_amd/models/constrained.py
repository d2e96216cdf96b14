"""Decoding inside a closed answer set: the static form of HF's ``prefix_allowed_tokens_fn`` (``PrefixConstrainedLogitsProcessor``,
transformers/generation/logits_process.py:1484-1553), for the encoder-decoder (``VCT0Model.generate``) and the causal
(``ClipCaptionModel.generate`` / ``generate_fewshot`` / ``generate_beams*`` / ``generate_draws*``) path.

A constraint is a set of token-id sequences, shared by all items of a batch or one set per item (an item's beams or draws share its
set).  The host builds the set's trie ONCE per ``generate`` call (:class:`AnswerTrie`, CSR arrays); every decoder step then runs one
``eavqa_trie_constrain`` on the step's scores, after ``eavqa_logits_process`` and before the pick - HF's place for this processor
(generation/utils.py:1239-1245).  The kernel walks a row's generated ids from the item's root, so nothing has to follow a beam reorder.
The callback this equals: ``[eos]`` once a row has ended or left the set, else the node's children, plus eos where a member ends.
Without the keyword there is no trie, no allocation and no launch."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .logits_process import _index

CONSTRAINT_KWARGS = ("allowed_sequences",)
MAX_SEQUENCE_LENGTH = 64          # tokens per member: the depth of the walk eavqa_trie_constrain redoes every step
MAX_TOTAL_TOKENS = 1 << 20        # tokens over all members of all sets (the CSR arrays stay a few MB)
LDS_CHILDREN = 2048               # TC_LDS_CHILDREN of csrc/constrain.hip: a node's child list up to this long is searched in LDS
EXCLUDED_KWARGS = ("no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens")
PAD_LABEL = -100


def _check_set(seqs, what: str) -> List[Tuple[int, ...]]:
    if not isinstance(seqs, (list, tuple)) or len(seqs) == 0:
        raise ValueError(f"allowed_sequences: {what} is empty: a non-empty list of non-empty lists of token ids")
    out = []
    for s in seqs:
        if not isinstance(s, (list, tuple)) or len(s) == 0:
            raise ValueError(f"allowed_sequences: {what} holds an empty sequence (or something that is no list): {s!r}")
        ids = tuple(_index(t) for t in s)
        if any(t is None for t in ids):
            raise ValueError(f"allowed_sequences: {what} holds a non-integer id in {list(s)!r}")
        if any(t < 0 for t in ids):
            raise ValueError(f"allowed_sequences: {what} holds an id < 0 in {list(s)!r}")
        if len(ids) > MAX_SEQUENCE_LENGTH:
            raise NotImplementedError(f"allowed_sequences: a sequence of {len(ids)} tokens; at most MAX_SEQUENCE_LENGTH = "
                                      f"{MAX_SEQUENCE_LENGTH} are built")
        out.append(ids)
    return list(dict.fromkeys(out))                                     # duplicates collapse


class AnswerTrie:
    """The trie of a constraint in CSR form, on the host.  ``sequences``: one set for every item; ``per_item``: one set per item (then
    ``roots`` int32 [B] names each item's root node, else it is None and the root is node 0).  Node i's children are the edges
    ``child_begin[i] : child_begin[i + 1]``, edge e carries token ``child_tok[e]`` (ascending within a node) to node ``child_node[e]``;
    ``is_end[i]``: a member ends at node i.  ``sets`` keeps the members per item (one entry when shared), duplicates collapsed."""

    def __init__(self, sequences=None, per_item=None, eos_token_id: Optional[int] = None):
        if (sequences is None) == (per_item is None):
            raise ValueError("allowed_sequences: give `sequences` (one set for all items) or `per_item` (one set per item)")
        if per_item is not None:
            if not isinstance(per_item, (list, tuple)) or len(per_item) == 0:
                raise ValueError("allowed_sequences: per_item is empty: one non-empty set per item")
            self.sets = [_check_set(s, f"the set of item {i}") for i, s in enumerate(per_item)]
        else:
            self.sets = [_check_set(sequences, "the set")]
        self.n_items: Optional[int] = len(self.sets) if per_item is not None else None
        self.n_tokens = sum(len(s) for st in self.sets for s in st)
        if self.n_tokens > MAX_TOTAL_TOKENS:
            raise NotImplementedError(f"allowed_sequences: {self.n_tokens} tokens in total; at most 2**20 are built")
        self.max_id = max(t for st in self.sets for s in st for t in s)
        self.eos_token_id = None if eos_token_id is None else int(eos_token_id)
        # nodes in creation order (the roots first, then depth-first along the insertions); children kept as dicts until the CSR pass
        kids: List[dict] = [dict() for _ in self.sets]
        end: List[int] = [0] * len(self.sets)
        for root, st in enumerate(self.sets):
            for s in st:
                node = root
                for t in s:
                    nxt = kids[node].get(t)
                    if nxt is None:
                        nxt = len(kids)
                        kids[node][t] = nxt
                        kids.append(dict())
                        end.append(0)
                    node = nxt
                end[node] = 1
        begin, tok, dst = [0], [], []
        for ch in kids:
            for t in sorted(ch):
                tok.append(t)
                dst.append(ch[t])
            begin.append(len(tok))
        self.child_begin = torch.tensor(begin, dtype=torch.int32)
        self.child_tok = torch.tensor(tok, dtype=torch.int32)
        self.child_node = torch.tensor(dst, dtype=torch.int32)
        self.is_end = torch.tensor(end, dtype=torch.uint8)
        self.roots = torch.arange(len(self.sets), dtype=torch.int32) if per_item is not None else None

    @classmethod
    def from_candidates(cls, candidates, eos_token_id: Optional[int] = None) -> "AnswerTrie":
        """From the tensor ``score_candidates`` takes: int64 [C, Tc] (one set for all items) or [B, C, Tc] (one per item), right-padded
        with -100.  A candidate may end in ``eos_token_id`` (appended there to have it scored): that last token is dropped here, the set
        holds the answer alone."""
        cand = torch.as_tensor(candidates)
        if cand.dtype not in (torch.int64, torch.int32) or cand.dim() not in (2, 3):
            raise ValueError(f"allowed_sequences: candidates are integer ids [C, Tc] or [B, C, Tc] (got {cand.dtype} {tuple(cand.shape)})")
        host = cand.detach().to("cpu", torch.int64)

        def one(rows) -> List[List[int]]:
            out = []
            for r in rows.tolist():
                s = r[:r.index(PAD_LABEL)] if PAD_LABEL in r else r
                if eos_token_id is not None and len(s) > 1 and s[-1] == int(eos_token_id):
                    s = s[:-1]
                out.append(s)
            return out
        if host.dim() == 2:
            return cls(sequences=one(host), eos_token_id=eos_token_id)
        return cls(per_item=[one(h) for h in host], eos_token_id=eos_token_id)

    @classmethod
    def coerce(cls, value) -> "AnswerTrie":
        """What the ``allowed_sequences`` keyword takes: an :class:`AnswerTrie`, a list of id lists, or a list of such lists per item."""
        if isinstance(value, AnswerTrie):
            return value
        if isinstance(value, torch.Tensor):
            return cls.from_candidates(value)
        if not isinstance(value, (list, tuple)) or len(value) == 0:
            raise ValueError(f"allowed_sequences={value!r}: the set is empty: an AnswerTrie, a non-empty list of id lists, or one such "
                             "list per item")
        nested = any(isinstance(s, (list, tuple)) and len(s) > 0 and isinstance(s[0], (list, tuple)) for s in value)
        return cls(per_item=list(value)) if nested else cls(sequences=list(value))

    def bound(self, eos_token_id: int, batch_size: Optional[int] = None) -> "AnswerTrie":
        """This trie checked against the eos id of a call (no member may hold it: eos is what ENDS a member) and its batch size."""
        eos = int(eos_token_id)
        for i, st in enumerate(self.sets):
            for s in st:
                if eos in s:
                    raise ValueError(f"allowed_sequences: {list(s)} contains eos_token_id={eos}" + (f" (item {i})" if self.n_items else "")
                                     + ": eos ends a member, it is not part of one")
        self.check_items(batch_size)
        if self.eos_token_id == eos:
            return self
        other = object.__new__(AnswerTrie)
        other.__dict__.update(self.__dict__)
        other.eos_token_id = eos
        return other

    def check_items(self, batch_size: Optional[int]) -> None:
        if batch_size is not None and self.n_items is not None and self.n_items != int(batch_size):
            raise ValueError(f"allowed_sequences: per_item holds {self.n_items} sets for a batch of {int(batch_size)} items")

    def upload(self, V: int, device) -> "DeviceTrie":
        return DeviceTrie(self, V, device)


class DeviceTrie:
    """An :class:`AnswerTrie` on the device: built ONCE per ``generate`` call, never per step."""

    def __init__(self, trie: AnswerTrie, V: int, device):
        if trie.eos_token_id is None:
            raise ValueError("allowed_sequences without an eos_token_id: there is no token to end a member with")
        if trie.max_id >= V:
            over = sorted({t for st in trie.sets for s in st for t in s if t >= V})
            raise ValueError(f"allowed_sequences: the vocabulary holds {V} tokens, but {over[:8]} were named")
        if not 0 <= trie.eos_token_id < V:
            raise ValueError(f"allowed_sequences: eos_token_id={trie.eos_token_id} is outside the vocabulary of {V} tokens")
        self.trie, self.eos = trie, trie.eos_token_id
        self.child_begin, self.child_tok = trie.child_begin.to(device), trie.child_tok.to(device)
        self.child_node, self.is_end = trie.child_node.to(device), trie.is_end.to(device)
        self.roots = trie.roots.to(device) if trie.roots is not None else None

    def apply(self, scores, V: int, history, cur_len: int, prompt_len: int, to_logprobs: bool = False) -> None:
        """The mask for the step that follows a history of ``cur_len`` ids (the first ``prompt_len`` of them are no generated ids), in
        place on ``scores`` float32 [R, >= V].  With one set per item, the R rows are the items' beams or draws, ordered (item, row)."""
        from .. import ops
        rows = 1
        if self.roots is not None:
            n = self.trie.n_items
            if scores.shape[0] % n:
                raise ValueError(f"allowed_sequences: per_item holds {n} sets, which does not divide the {scores.shape[0]} decoder rows")
            rows = scores.shape[0] // n
        ops.trie_constrain(scores, V, history, cur_len, prompt_len, self.eos, self.child_begin, self.child_tok, self.child_node, self.is_end,
                           roots=self.roots, rows_per_item=rows, to_logprobs=to_logprobs)


def constraint_plan(kw: dict) -> Optional[AnswerTrie]:
    """``kw``: generation arguments by name - ``allowed_sequences`` (missing or None = no constraint), the logits-processor names, plus
    ``eos_token_id`` (one id or None) as the path resolved it and ``batch_size`` (None = checked later, by
    :meth:`AnswerTrie.check_items`).  None without a constraint, else the :class:`AnswerTrie` bound to the eos id."""
    value = kw.get("allowed_sequences")
    if value is None:
        return None
    for name in EXCLUDED_KWARGS:
        if kw.get(name):
            raise NotImplementedError(f"{name} together with allowed_sequences is not built: the rule could leave a row without an "
                                      "allowed token, and the set already fixes the lengths")
    trie = AnswerTrie.coerce(value)
    eos = kw.get("eos_token_id")
    if eos is None:
        raise ValueError("allowed_sequences without an eos_token_id: there is no token to end a member with")
    return trie.bound(int(eos), kw.get("batch_size"))


def upload_constraint(constraint: Optional[AnswerTrie], eos_token_id: Optional[int], batch_size: int, V: int, device) -> Optional[DeviceTrie]:
    """What a decoding loop does with its ``constraint=`` argument before the first step: None stays None (nothing is allocated), a trie is
    checked against the loop's own eos id and batch size and put on the device."""
    if constraint is None:
        return None
    if eos_token_id is None or int(eos_token_id) < 0:
        raise ValueError("allowed_sequences without an eos_token_id: there is no token to end a member with")
    return constraint.bound(int(eos_token_id), batch_size).upload(V, device)


def split_constraint_kwargs(kw: dict) -> Tuple[dict, dict]:
    """``kw`` without the constraint argument, and that argument (for a path whose other checks reject names they do not know)."""
    return {k: v for k, v in kw.items() if k not in CONSTRAINT_KWARGS}, {k: v for k, v in kw.items() if k in CONSTRAINT_KWARGS}
