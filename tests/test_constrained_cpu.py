"""CPU: decoding inside a closed answer set.  tests/_constrained_ref.py (what the GPU tests compare ``eavqa_trie_constrain`` with)
equals HF's ``PrefixConstrainedLogitsProcessor`` bit for bit; the host side (``AnswerTrie``, ``constraint_plan``, the plans of both
generate paths) keeps its invariants and raises what it promises; ``eavqa_trie_constrain`` validates before any launch; and the
committed fixture tests/golden/constrained.npz holds what tests/golden/make_golden_constrained.py promises."""
import numpy as np
import pytest
import torch

import _constrained_ref as ref
from conftest import load_golden

EOS = 1
SET = [[5], [5, 9], [5, 9, 3], [5, 4], [7], [7, 7, 2, 6], [8, 11]]            # "new" / "new york": [5] ends AND continues


def _histories(P):
    """(name, generated ids) of the four kinds: empty, on an end node with children, ended and followed by pads, off the trie."""
    return [("empty", []), ("end_with_children", [5]), ("inner", [7, 7]), ("leaf", [8, 11]), ("ended_pads", [5, 9, EOS, 0, 0]),
            ("off", [5, 6]), ("off_first", [12]), ("eos_first", [EOS]), ("past_leaf", [8, 11, 4])]


# ------------------------------------------------------------------------------------------------ the restatement against HF
@pytest.mark.parametrize("P", [0, 1])
@pytest.mark.parametrize("num_beams", [1, 3])
def test_mask_equals_hf_prefix_constrained_processor(P, num_beams):
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    V = 16
    gen = torch.Generator().manual_seed(3)
    per_item = [SET, [[2], [2, 3]], [[10, 10, 10]]]
    for name, body in _histories(P):
        for shared, items in ((SET, None), (None, per_item)):
            R = 3 * num_beams
            scores = torch.randn(R, V, generator=gen)
            hist = torch.tensor([[0] * P + body] * R, dtype=torch.int64)
            if body:                                                        # the rows differ: row 1 takes another turn at its last id
                hist[1, -1] = 9
            cur = hist.shape[1]
            fn = ref.allowed_fn(EOS, P, shared, items)
            want = PrefixConstrainedLogitsProcessor(fn, num_beams)(hist, scores.clone())
            got = ref.mask(scores, hist, P, cur, EOS, shared, items)
            assert torch.equal(got, want), (name, shared is None)
            assert bool(torch.isfinite(got).any(dim=1).all())               # no row is left empty
            keep = torch.isfinite(got)
            assert torch.equal(got[keep], scores[keep])                     # allowed columns keep their bits
            lp = ref.mask(scores, hist, P, cur, EOS, shared, items, to_logprobs=True)
            assert torch.equal(lp, PrefixConstrainedLogitsProcessor(fn, num_beams)(hist, torch.log_softmax(scores, -1)))


def test_walk_by_definition():
    assert ref.walk(SET, [], EOS) == [5, 7, 8]
    assert ref.walk(SET, [5], EOS) == [EOS, 4, 9]
    assert ref.walk(SET, [5, 9, 3], EOS) == [EOS]
    assert ref.walk(SET, [7, 7], EOS) == [2]
    assert ref.walk(SET, [5, 9, EOS, 0, 0], EOS) == [EOS] and ref.walk(SET, [6], EOS) == [EOS]


# ------------------------------------------------------------------------------------------------ AnswerTrie
def _walk_trie(t, root, history, eos):
    """The allowed set read off the CSR arrays on the host, the way the kernel walks them."""
    b, tok, dst, end = t.child_begin.tolist(), t.child_tok.tolist(), t.child_node.tolist(), t.is_end.tolist()
    node = root
    for h in history:
        kids = tok[b[node]:b[node + 1]]
        if h not in kids:
            return [eos]
        node = dst[b[node] + kids.index(h)]
    out = tok[b[node]:b[node + 1]] + ([eos] if end[node] or b[node] == b[node + 1] else [])
    return sorted(out)


def test_answer_trie_csr_invariants():
    from eavqa_amd.models.constrained import AnswerTrie
    t = AnswerTrie(sequences=SET + [[5, 9], [7]])                            # duplicates collapse
    assert t.sets == [[tuple(s) for s in SET]] and t.roots is None and t.n_items is None
    b, tok = t.child_begin.tolist(), t.child_tok.tolist()
    N = t.is_end.numel()
    assert t.child_begin.dtype == t.child_tok.dtype == t.child_node.dtype == torch.int32 and t.is_end.dtype == torch.uint8
    assert len(b) == N + 1 and b[0] == 0 and b[-1] == len(tok) == t.child_node.numel() == N - 1           # a tree: one edge into every node but the root
    assert all(b[i] <= b[i + 1] for i in range(N))
    for i in range(N):
        kids = tok[b[i]:b[i + 1]]
        assert kids == sorted(set(kids))                                     # ascending, distinct
    assert sorted(t.child_node.tolist()) == list(range(1, N))
    assert int(t.is_end.sum()) == len(SET)
    for name, body in _histories(0):
        assert _walk_trie(t, 0, body, EOS) == ref.walk(SET, body, EOS), name
    assert N == 1 + len({tuple(s[:i]) for s in SET for i in range(1, len(s) + 1)})


def test_answer_trie_per_item_roots_and_from_candidates():
    from eavqa_amd.models.constrained import AnswerTrie
    per_item = [SET, [[2], [2, 3]], [[10, 10, 10]]]
    t = AnswerTrie(per_item=per_item)
    assert t.n_items == 3 and t.roots.tolist() == [0, 1, 2] and t.roots.dtype == torch.int32
    for i, st in enumerate(per_item):
        for body in ([], [5], [2], [10, 10], [2, 3], [9]):
            assert _walk_trie(t, i, body, EOS) == ref.walk(st, body, EOS), (i, body)
    cand = torch.full((len(SET), 5), -100, dtype=torch.int64)
    for i, s in enumerate(SET):
        cand[i, :len(s)] = torch.tensor(s)
    a, b = AnswerTrie.from_candidates(cand), AnswerTrie(sequences=SET)
    for f in ("child_begin", "child_tok", "child_node", "is_end"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    three = AnswerTrie.from_candidates(cand.unsqueeze(0).repeat(2, 1, 1))
    assert three.n_items == 2 and three.sets[0] == three.sets[1] == b.sets[0]
    with_eos = cand.clone()
    with_eos[0, 1] = EOS                                                     # [5, eos]: the form score_candidates scores eos with
    assert AnswerTrie.from_candidates(with_eos, eos_token_id=EOS).sets == b.sets
    assert AnswerTrie.coerce(SET).sets == b.sets and AnswerTrie.coerce(per_item).n_items == 3 and AnswerTrie.coerce(b) is b


# ------------------------------------------------------------------------------------------------ what raises
def _plan(**kw):
    from eavqa_amd.models.constrained import constraint_plan
    return constraint_plan(dict(dict(eos_token_id=EOS), **kw))


@pytest.mark.parametrize("value,match", [
    ([], "empty"),
    ([SET, []], "item 1 is empty"),
    ([[5], []], "empty sequence"),
    ([[5, 2.5]], "non-integer"),
    ([[5, True]], "non-integer"),
    ([[5, -3]], "id < 0"),
    ([[5, EOS]], "contains eos_token_id"),
])
def test_constraint_plan_value_errors(value, match):
    with pytest.raises(ValueError, match=f"allowed_sequences.*{match}"):
        _plan(allowed_sequences=value)


def test_constraint_plan_other_errors():
    from eavqa_amd.models.constrained import MAX_SEQUENCE_LENGTH, AnswerTrie
    assert _plan() is None and _plan(allowed_sequences=None, min_length=3) is None
    with pytest.raises(ValueError, match="allowed_sequences without an eos_token_id"):
        _plan(allowed_sequences=SET, eos_token_id=None)
    with pytest.raises(ValueError, match="per_item holds 2 sets for a batch of 3"):
        _plan(allowed_sequences=[SET, SET], batch_size=3)
    assert _plan(allowed_sequences=[SET, SET], batch_size=2).n_items == 2
    assert MAX_SEQUENCE_LENGTH == 64
    assert _plan(allowed_sequences=[list(range(2, 66))]).n_tokens == 64
    with pytest.raises(NotImplementedError, match="allowed_sequences.*MAX_SEQUENCE_LENGTH"):
        _plan(allowed_sequences=[list(range(2, 67))])
    big = [[2 + (i % 1000), 2 + (i // 1000), 2 + j] for i in range(2 ** 18 // 2) for j in range(3)]           # 1.18e6 tokens
    with pytest.raises(NotImplementedError, match=r"allowed_sequences.*2\*\*20"):
        _plan(allowed_sequences=big)
    for name, v in (("no_repeat_ngram_size", 2), ("bad_words_ids", [[4]]), ("min_length", 3), ("min_new_tokens", 2)):
        with pytest.raises(NotImplementedError, match=name):
            _plan(allowed_sequences=SET, **{name: v})
    assert _plan(allowed_sequences=SET, repetition_penalty=1.3, no_repeat_ngram_size=0).eos_token_id == EOS
    with pytest.raises(ValueError, match=r"vocabulary holds 10 tokens.*\[11\]"):                               # at upload, like bad words
        AnswerTrie(sequences=SET, eos_token_id=EOS).upload(10, "cpu")


def test_both_generate_plans_accept_the_keyword_and_only_then_hold_a_constraint():
    from eavqa_amd.models.constrained import AnswerTrie
    from eavqa_amd.models.decode import shared_search_plan
    from eavqa_amd.models.vct0 import generation_plan
    assert "constraint" not in generation_plan(dict(num_beams=2), config_eos_token_id=EOS)
    p = generation_plan(dict(num_beams=4, allowed_sequences=SET, repetition_penalty=1.2), max_length=8, config_eos_token_id=EOS)
    assert isinstance(p["constraint"], AnswerTrie) and p["constraint"].eos_token_id == EOS and p["logits"].repetition_penalty == 1.2
    assert generation_plan(dict(allowed_sequences=SET, eos_token_id=13), config_eos_token_id=EOS)["constraint"].eos_token_id == 13
    assert generation_plan(dict(do_sample=True, num_return_sequences=4, allowed_sequences=AnswerTrie(sequences=SET)),
                           config_eos_token_id=EOS)["constraint"].sets == AnswerTrie(sequences=SET).sets
    with pytest.raises(NotImplementedError, match="min_length"):
        generation_plan(dict(allowed_sequences=SET, min_length=2), max_length=8, config_eos_token_id=EOS)
    with pytest.raises(ValueError, match="contains eos_token_id"):
        generation_plan(dict(allowed_sequences=[[5, 3]], eos_token_id=3), config_eos_token_id=EOS)
    with pytest.raises(NotImplementedError, match="prefix_allowed_tokens_fn"):                                 # the callback itself stays out
        generation_plan(dict(prefix_allowed_tokens_fn=lambda b, i: [1]), config_eos_token_id=EOS)
    for kind, extra in (("beams", dict(num_beams=3)), ("draws", dict(num_return_sequences=4))):
        assert "constraint" not in shared_search_plan(kind, dict(extra), config_eos_token_id=EOS, config_pad_token_id=0)
        q = shared_search_plan(kind, dict(extra, allowed_sequences=SET), config_eos_token_id=EOS, config_pad_token_id=0)
        assert q["constraint"].eos_token_id == EOS
        with pytest.raises(NotImplementedError, match="bad_words_ids"):
            shared_search_plan(kind, dict(extra, allowed_sequences=SET, bad_words_ids=[[4]]), config_eos_token_id=EOS, config_pad_token_id=0)
        with pytest.raises(ValueError, match="without an eos_token_id"):
            shared_search_plan(kind, dict(extra, allowed_sequences=SET), config_eos_token_id=None, config_pad_token_id=0)


# ------------------------------------------------------------------------------------------------ the C entry validates on the host
def _entry(lib, **over):
    a = dict(R=6, V=64, scores=16, ld=64, to_logprobs=0, history=16, ld_history=8, prompt_len=1, cur_len=3, eos=1, child_begin=16, child_tok=16,
             child_node=16, is_end=16, n_nodes=4, n_edges=3, roots=None, rows_per_item=1, stream=None)
    assert not set(over) - set(a), over
    a.update(over)
    return lib.eavqa_trie_constrain(*[a[n] for n in ("R", "V", "scores", "ld", "to_logprobs", "history", "ld_history", "prompt_len", "cur_len", "eos",
                                                     "child_begin", "child_tok", "child_node", "is_end", "n_nodes", "n_edges", "roots",
                                                     "rows_per_item", "stream")])


@pytest.mark.parametrize("fault,code", [
    (dict(scores=None), -1), (dict(R=0), -1), (dict(V=0), -1), (dict(to_logprobs=2), -1), (dict(history=None), -1),
    (dict(prompt_len=4), -1), (dict(prompt_len=-1), -1), (dict(eos=-1), -1), (dict(eos=64), -1), (dict(child_begin=None), -1),
    (dict(child_tok=None), -1), (dict(child_node=None), -1), (dict(is_end=None), -1), (dict(n_nodes=0), -1), (dict(n_edges=-1), -1),
    (dict(rows_per_item=0), -1), (dict(ld=60), -3), (dict(ld_history=2), -3), (dict(rows_per_item=4, roots=16), -3),
])
def test_trie_constrain_rejects_bad_arguments_before_any_launch(fault, code):
    from eavqa_amd import build, _lib
    build.build()
    assert _entry(_lib.load(), **fault) == code


# ------------------------------------------------------------------------------------------------ the fixture
def _fixture_sets(f):
    sets = [[[int(t) for t in m if t >= 0] for m in st if m[0] >= 0] for st in f("sets")]
    return (sets[0], None) if int(f("params")[5]) == 0 else (None, sets)


def test_fixture_is_sane():
    z = load_golden("constrained.npz")
    cases = z["cases"].tolist()
    assert {"g_shared", "b4_shared", "b4_item", "b4_short", "g_rp", "g_cut"} <= set(cases)
    for family, start in (("t5", 1), ("causal", 0)):
        for tag in z[family].tolist():
            for name in cases:
                f = lambda field: z[f"{tag}.{name}.{field}"]
                k, nrs, n_new, eos, pad, per = [int(v) for v in f("params")]
                shared, per_item = _fixture_sets(f)
                seq = f("sequences")
                assert float(f("min_gap")) >= 1e-3, (tag, name)
                assert seq.shape[0] % (nrs if k > 1 else 1) == 0 and seq.shape[1] <= n_new + start
                sets = ref.item_sets(shared, per_item, seq.shape[0])
                some_cut = False
                for r, row in enumerate(seq.tolist()):
                    body, full = ref.cut(row, eos, start), eos in row[start:]
                    some_cut = some_cut or not full
                    assert any((m == body) if full else (m[:len(body)] == body and len(body) == n_new) for m in sets[r]), (tag, name, row)
                assert some_cut == name.endswith("_cut"), (tag, name)
                if k > 1:
                    assert np.isfinite(f("sequences_scores")).all() and f("sequences_scores").shape == (seq.shape[0],)
                if name == "b4_short":
                    assert nrs == 2 and min(len(s) for s in per_item) == 2
                if name == "b4_shared":                                      # the strict-prefix pair is in the set
                    assert any(a != b and b[:len(a)] == a for a in shared for b in shared) and len(shared) == 12
