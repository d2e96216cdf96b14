"""GPU: exact probes for ``eavqa_trie_constrain`` (csrc/constrain.hip) on RAW CSR arrays - tables ``AnswerTrie`` never builds.

The cases and the reference (``trie_keep``: the contract of include/eavqa.h restated on raw arrays, clamps included) are
tests/_answer_probe.py; tests/test_answer_probe_cpu.py shows that the reference is tests/_constrained_ref.py on well-formed tables, that
no damaged table can send even an unguarded kernel outside its buffers, and that each case is not vacuous.  Calls go through ctypes:
every array is a window inside a larger device buffer.  The acceptance is exact, as in tests/test_constrain_kernel_gpu.py:
``to_logprobs = 0``: -inf where the reference removes a column, the input's own bits elsewhere; ``to_logprobs = 1``: the bits
``eavqa_logits_process(to_logprobs=1)`` leaves on the same row; columns in [V, ld), the buffer around the view, the history and every
table buffer are bit-unchanged; no row is left without a finite column.

The header's contract, sentence by sentence, and the case that executes it (ids are ``test_trie_cases[name-to_logprobs]``), with the
mutation that turns it red ("run" = built into a scratch copy of the library and run once on the MI355X; "read" = argued from the code,
never run: it moves an address):
  "Indices outside the arrays are never followed"
      roots[] outside [0, n_nodes)            root_minus1, root_n_nodes, rows_per_item3      without `node >= 0 && node < n_nodes` the
                                              kernel reads child_begin[-1] / [n_nodes + 1]   (read)
      child_node[] outside [0, n_nodes)       child_node_minus1, child_node_n_nodes          the same test after `node = child_node[lo]` (read)
      child_begin below 0 / above n_edges / decreasing
                                              begin_minus3, begin_past_edges, begin_decreasing      without the two clamps of `children`
                                              the list starts 3 ids in front of child_tok, 5 behind it, or has a negative length  (read)
  "A history id is compared as int64"         wide_ids      `(int64_t)child_tok[mid] < tok` and `== tok` -> `child_tok[..] < (int32_t)tok`
                                              (run: wide_ids-0 and wide_ids-1 red - the rows holding 2**32 + t and t - 2**32 come
                                              back as the row holding t; the 28 others green)
  "eos_token_id when is_end is set there (or the node has no child)"
                                              no_edges-end0 (n_edges = 0, child_tok = child_node = NULL), the leaf with is_end = 0 of
                                              the damaged tables      `n == 0 ||` removed: the row would be all -inf   (read: it needs
                                              no run - `assert keep.any(1)` of every case is the same statement)
  "A child list of up to 2048 ids is searched in LDS, a longer one in global memory", at a node reached by a walk
                                              fan2048, fan2049      `n <= TC_LDS_CHILDREN` -> `n < TC_LDS_CHILDREN` only moves the
                                              boundary (same values); the staging loop `i += BR_THREADS` taken once loses the ids
                                              behind the 1024th of fan2048 (read)
  the walk: "Row r's generated ids ... are walked from the root", the row that consumed eos has ended
                                              chain40 (40 ids deep; a wrong id at position 20; eos in the middle with the true
                                              continuation behind it)   (read: a walk that skipped eos would allow CHAIN[38])
  "ascending and distinct within a node" - what the code does when an id repeats
                                              duplicate     the merge's `while (.. < c) ++lo` -> `if`: the 10 of [8, 9, 9, 10] is lost
                                              (read); the walk takes the FIRST of the two edges (the lower bound)
  "roots ... one set per item, shared by the item's rows_per_item beams"
                                              rows_per_item3: `row / rows_per_item` -> `row` would read roots[3 ..] (read)
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _answer_probe as P

DEV = "cuda"
POISON = 12345.0
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import _lib
    lib = _lib.load()
    assert lib.eavqa_check_device() == 0, "not a gfx950 device"
    return lib


def _window_ptr(dev, off):
    return ctypes.c_void_p(dev.data_ptr() + off * dev.element_size())


@pytest.mark.parametrize("to_logprobs", [0, 1])
@pytest.mark.parametrize("name", [c.name for c in P.trie_cases()])
def test_trie_cases(lib, name, to_logprobs):
    from eavqa_amd import ops
    c = P.trie_case(name)
    t = c.table
    V, ld = c.V, c.ld
    host = dict(cb=t.cb_buf, tok=t.tok_buf, node=t.node_buf, end=t.end_buf)
    if c.roots_buf is not None:
        host["roots"] = c.roots_buf
    dev = {n: torch.from_numpy(a).to(DEV) for n, a in host.items()}
    tok_ptr = None if t.null_edges else _window_ptr(dev["tok"], t.tok_off)
    node_ptr = None if t.null_edges else _window_ptr(dev["node"], t.node_off)
    roots_ptr = _window_ptr(dev["roots"], c.roots_off) if "roots" in dev else None
    for call, rows in enumerate(c.calls):
        R, cur = len(rows), c.prompt_len + len(rows[0])
        hist_h = torch.from_numpy(P.history_rows(c, rows))
        hist = hist_h.to(DEV)
        keep = torch.from_numpy(P.trie_keep(c, rows))
        assert bool(keep.any(dim=1).all())
        gen = torch.Generator().manual_seed(1000 * call + to_logprobs)
        flat_h = torch.full(((R + 2) * ld,), POISON)
        flat_h[ld:ld + R * ld].view(R, ld)[:, :V] = 4.0 * torch.randn(R, V, generator=gen)
        flat = flat_h.to(DEV)
        view = flat[ld:ld + R * ld].view(R, ld)
        source = view[:, :V].cpu()
        if to_logprobs:
            lp = view.clone()
            ops.logits_process(lp, V, None, 0, to_logprobs=True)                    # no rule: log_softmax alone
            source = lp[:, :V].cpu()
        want = torch.where(keep, source, torch.full_like(source, -INF))
        rc = lib.eavqa_trie_constrain(R, V, ctypes.c_void_p(view.data_ptr()), ld, to_logprobs, ctypes.c_void_p(hist.data_ptr()), hist.stride(0),
                                      c.prompt_len, cur, P.EOS, _window_ptr(dev["cb"], t.cb_off), tok_ptr, node_ptr,
                                      _window_ptr(dev["end"], t.end_off), t.n_nodes, t.n_edges, roots_ptr, c.rows_per_item, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        after = flat.cpu()
        got = after[ld:ld + R * ld].view(R, ld)[:, :V]
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        assert bad.numel() == 0, (call, bad[:8].tolist())
        assert bool(torch.isfinite(got).any(dim=1).all()), call
        outside = torch.ones(flat_h.numel(), dtype=torch.bool)
        outside[ld:ld + R * ld].view(R, ld)[:, :V] = False
        assert torch.equal(after[outside].view(torch.int32), flat_h[outside].view(torch.int32)), call     # [V, ld) and around the view
        assert torch.equal(hist.cpu(), hist_h), call
    for n, a in host.items():
        assert np.array_equal(dev[n].cpu().numpy(), a), n
