"""GPU: ``eavqa_trie_constrain`` against tests/_constrained_ref.py (which tests/test_constrained_cpu.py pins to HF's
``PrefixConstrainedLogitsProcessor``).  Without ``to_logprobs`` the result is EXACT: -inf where the reference has it, the input's bits
elsewhere.  With it, an allowed column holds the bits ``eavqa_logits_process(to_logprobs=1)`` leaves on the same row.  Columns in
[V, ld) are poisoned before every call and must come back unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _constrained_ref as ref

DEV = "cuda"
EOS, PAD = 1, 2
POISON = 12345.0


def _mixed(V):
    """A leaf that is only an end node ([V-1, 0] under V-1), a one-child node ([7] -> 7), an end node with children ([5]), children 0 and
    V - 1 (at the root and below), a member of 5 ids."""
    return [[0], [V - 1, 0], [V - 1, V - 1, 9], [5], [5, 0], [5, V - 1], [5, 9, 3], [7, 7, 6, 4, 8], [V - 2, 3]]


def _histories(members, L, n, seed):
    """``n`` generated-id rows of exactly ``L`` ids covering the four kinds: on the trie (every prefix of length L: inner nodes, end nodes
    with children, leaves), ended (a member, eos, pads), eos behind a non-member prefix (left the set), and off-trie ids."""
    if L == 0:
        return [[] for _ in range(n)]
    gen = torch.Generator().manual_seed(seed)
    pool = [list(p) for p in sorted({tuple(m[:L]) for m in members if len(m) >= L})]
    pool += [m + [EOS] + [PAD] * (L - len(m) - 1) for m in members if len(m) < L]
    is_member = {tuple(m) for m in members}
    early = (m[:j] + [EOS] + [PAD] * (L - j - 1) for m in members for j in range(min(len(m), L)) if tuple(m[:j]) not in is_member)
    pool += [h for h, _ in zip(early, range(4))]
    pool += [torch.randint(3, 60, (L,), generator=gen).tolist() for _ in range(2)]
    pool += [m[:L - 1] + [4] for m in members if len(m) >= L][:2]                                     # leaves at the last id
    return [pool[i % len(pool)] for i in range(n)]


def _scores(R, V, ld, offset, seed):
    """float32 [R, V] view with row stride ``ld`` starting ``offset`` floats into a poisoned flat buffer."""
    gen = torch.Generator().manual_seed(seed)
    flat = torch.full((R * ld + offset + 4,), POISON, dtype=torch.float32)
    view = flat[offset:offset + R * ld].view(R, ld)
    view[:, :V] = 4.0 * torch.randn(R, V, generator=gen)
    flat = flat.to(DEV)
    return flat, flat[offset:offset + R * ld].view(R, ld)


def _check(V, ld, R, offset, P, sequences=None, per_item=None, lengths=(0, 1, 2, 3, 5), seed=0):
    from eavqa_amd import ops
    from eavqa_amd.models.constrained import AnswerTrie
    trie = AnswerTrie(sequences=sequences, per_item=per_item, eos_token_id=EOS).upload(V, DEV)
    sets = ref.item_sets(sequences, per_item, R)
    for L in lengths:
        bodies = [_histories(sets[r], L, R, seed + L)[r] for r in range(R)] if per_item is not None else _histories(sequences, L, R, seed + L)
        cur = P + L
        hist = torch.full((R, cur + 3), 77, dtype=torch.int64)                  # ids behind cur_len are never read: 77 is no member's id
        hist[:, :P] = 0
        for r, b in enumerate(bodies):
            hist[r, P:cur] = torch.tensor(b, dtype=torch.int64)
        hist_d = hist.to(DEV)
        for to_logprobs in (False, True):
            flat, view = _scores(R, V, ld, offset, seed + 100 * L)
            before = flat.clone()
            want = ref.mask(view[:, :V].cpu(), hist, P, cur, EOS, sequences, per_item)
            keep = torch.isfinite(want)
            assert bool(keep.any(dim=1).all())
            if to_logprobs:
                lp = view.clone()
                ops.logits_process(lp, V, hist_d, cur, to_logprobs=True)            # no rule: log_softmax alone
                want = torch.where(keep, lp[:, :V].cpu(), torch.full_like(want, float("-inf")))
            trie.apply(view, V, hist_d, cur, P, to_logprobs=to_logprobs)
            got = view[:, :V].cpu()
            assert torch.equal(got, want), (L, to_logprobs, (got != want).nonzero()[:8])
            if not to_logprobs:                                                     # allowed columns: the input's very bits
                assert torch.equal(got[keep].view(torch.int32), before[offset:offset + R * ld].view(R, ld)[:, :V].cpu()[keep].view(torch.int32))
            outside = torch.ones(flat.numel(), dtype=torch.bool)
            outside[offset:offset + R * ld].view(R, ld)[:, :V] = False
            assert torch.equal(flat.cpu()[outside], before.cpu()[outside]), (L, to_logprobs)      # [V, ld) and around the view


@pytest.mark.parametrize("P", [0, 1])
@pytest.mark.parametrize("V,ld,R,offset", [(1027, 1032, 70, 0), (4100, 4100, 1, 0), (6151, 6152, 70, 0), (1027, 1032, 3, 1), (1027, 1029, 3, 0)])
def test_kernel_matches_the_reference(V, ld, R, offset, P):
    """V 1027 in rows of 1032 (a scalar tail group), 4100 (a second column pass), 6151; 1 and 70 rows; a view one float off a 16-byte
    boundary and a row stride that is no multiple of 4 (both the scalar path)."""
    _check(V, ld, R, offset, P, sequences=_mixed(V))


@pytest.mark.parametrize("rows_per_item", [1, 3])
def test_per_item_roots(rows_per_item):
    V = 1027
    per_item = [_mixed(V), [[11], [11, 12]], [[0, V - 1, 0]], [[V - 1]], [[20, 21], [22], [20, 23, 24]]]
    _check(V, 1028, len(per_item) * rows_per_item, 0, 1, per_item=per_item)
    _check(V, 1028, len(per_item) * rows_per_item, 0, 0, per_item=per_item, lengths=(0, 2))


@pytest.mark.parametrize("V", [4100, 6151])
@pytest.mark.parametrize("extra", [0, 1])
def test_root_fan_out_at_and_above_the_lds_bound(V, extra):
    """The root's child list at exactly ``LDS_CHILDREN`` ids (searched in LDS) and one above (searched in global memory); the empty
    history reads the root's list, a one-id history a small list below it."""
    from eavqa_amd.models.constrained import LDS_CHILDREN, AnswerTrie
    gen = torch.Generator().manual_seed(V + extra)
    ids = sorted(set([0, V - 1] + [t for t in torch.randperm(V, generator=gen).tolist() if t not in (EOS, 0, V - 1)][:LDS_CHILDREN + extra - 2]))
    sequences = [[t] for t in ids[::2]] + [[t, 0] for t in ids[1::2]] + [[ids[3], V - 1], [ids[3], 5, 6]]
    trie = AnswerTrie(sequences=sequences)
    assert int(trie.child_begin[1] - trie.child_begin[0]) == LDS_CHILDREN + extra
    _check(V, V + (-V) % 4, 4, 0, 1, sequences=sequences, lengths=(0, 1, 2))


def test_wrapper_rejects_what_the_kernel_cannot_take():
    from eavqa_amd import _lib, ops
    from eavqa_amd.models.constrained import AnswerTrie
    t = AnswerTrie(per_item=[[[5]], [[6]]], eos_token_id=EOS).upload(64, DEV)
    s = torch.zeros((3, 64), device=DEV)
    h = torch.zeros((3, 2), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="does not divide"):
        t.apply(s, 64, h, 1, 1)
    with pytest.raises(_lib.EavqaError, match="float32 scores"):
        ops.trie_constrain(s.double(), 64, h, 1, 1, EOS, t.child_begin, t.child_tok, t.child_node, t.is_end)
    with pytest.raises(_lib.EavqaError, match="int64 history"):
        ops.trie_constrain(s, 64, h.int(), 2, 1, EOS, t.child_begin, t.child_tok, t.child_node, t.is_end)
    with pytest.raises(_lib.EavqaError, match="no CPU fallback"):
        ops.trie_constrain(s.cpu(), 64, h, 1, 1, EOS, t.child_begin, t.child_tok, t.child_node, t.is_end)
    with pytest.raises(_lib.EavqaError):                                            # eos outside [0, V): EAVQA_E_ARG
        ops.trie_constrain(s, 64, h, 1, 1, 64, t.child_begin, t.child_tok, t.child_node, t.is_end)
