"""No GPU: the cases of tests/_answer_probe.py are what their names say, their data is exact, their damaged tables cannot send an
unguarded kernel outside its buffers, ``trie_keep`` is tests/_constrained_ref.py on well-formed tables - and none of the probes is
vacuous: evaluating the references with one defect built in (``KILLERS``) changes what the named case expects on the GPU."""
import numpy as np
import pytest

import _answer_probe as P

JOINT = {c.name: c for c in P.joint_cases()}
TRIE = {c.name: c for c in P.trie_cases()}


# ================================================================================================ joint scores
def test_joint_grid_is_the_issues_grid_and_reaches_every_instantiation():
    shapes = {(c.D, c.k, c.Nq) for c in JOINT.values()}
    want = {(D, k, Nq) for D in (256, 260, 516, 1024, 1028, 1280) for k in (1, 5, 127, 128, 129) for Nq in (1, 3)} | {(16384, 9, 1), (16384, 9, 3)}
    assert shapes == want and len(JOINT) == 2 * len(want)
    assert {(c.D, c.k, c.Nq): 0 for c in JOINT.values() if c.kind == "query_onehot"}.keys() == want
    assert {P.js_nc(c.D) for c in JOINT.values()} == {0, 1, 4}                  # <2> and <3>: D = 512 / 768 of tests/test_rices_rerank_gpu.py
    assert all(c.Ni <= 40 for c in JOINT.values()) and 41 * (16384 + 12) * 4 < 3e6
    assert P.js_rj(260) == 8 and P.js_rj(1024) == 4 and 129 % 8 == 1 and 129 > P.JS_BLOCK      # the RJ = 8 tail in a second workgroup


def test_probe_columns_are_the_issues_columns():
    for D in (256, 260, 516, 1024, 1028, 1280, 16384):
        cols = set(P.probe_columns(D))
        must = {c for c in (0, 3, 4, 252, 255, 256, 259) if c < D} | {D - 4, D - 3, D - 2, D - 1}
        must |= {m for m in range(256, D, 256)} | {m - 1 for m in range(256, D, 256)}
        assert must <= cols and max(cols) == D - 1 and min(cols) == 0, D
    assert 256 not in P.probe_columns(256) and {256, 259} <= set(P.probe_columns(260)) and {1279, 1024, 1023} <= set(P.probe_columns(1280))


@pytest.mark.parametrize("name", list(JOINT))
def test_every_joint_case_pins_every_probe_column_with_exact_data(name):
    c = JOINT[name]
    pinned = set()
    for t in range(c.n_rounds):
        train, query, query_row, cols = c.round(t)
        pinned |= set(cols)
        if t in (0, c.n_rounds - 1):
            P.assert_joint_exact(c, train, query)
            assert train.shape == (c.Ni, c.D) and query.shape == (c.Nqi, c.D) and query_row.shape == (c.Nq,)
            assert (query_row >= 0).all() and (query_row < c.Nqi).all()
    assert pinned == set(c.cols)
    rows = c.image_rows()
    assert rows.shape == (c.Nq, c.k) and rows.min() >= 0 and rows.max() < c.Ni and c.text_idx.max() < c.Ndq
    assert not np.array_equal(c.text_idx[0], np.arange(c.k)) and rows[0, 0] != 0          # no identity; never train row 0 alone


def test_one_hot_probes_pin_one_element():
    c = JOINT["D260-k5-Nq3-query_onehot"]
    train, query, query_row, cols = c.round(5)
    joint, img = P.joint_reference(c, 5, "window")
    for i in range(c.Nq):
        assert (query[query_row[i]] != 0).sum() == 1 and query[query_row[i], cols[i]] == 1
        assert np.array_equal(img[i], train[c.image_rows()[i], cols[i]])
    assert np.array_equal(joint, c.text_sim + img)
    c = JOINT["D260-k5-Nq3-train_onehot"]
    train, query, query_row, cols = c.round(1)
    img = P.joint_reference(c, 1, "contiguous")[1]
    at = train.argmax(1)
    for i in range(c.Nq):
        v = c.image_rows()[i]
        assert np.array_equal(img[i], (v + 1) * query[query_row[i], at[v]])
    assert (query != 0).all() and (train != 0).sum() == c.Ni


def test_window_layout_pads_both_tables_differently():
    for D in (256, 16384):
        assert P.js_lds(D, "contiguous") == (D, D) and P.js_lds(D, "window") == (D + 4, D + 12)
    w = P.window(np.zeros((3, 8), np.float32), 12)
    assert w.shape == (4, 12) and (w[:3, 8:] == P.JS_PAD).all() and (w[3] == P.JS_PAD).all() and not w[:3, :8].any()


def _joint_differs(name, layout, defect):
    c = JOINT[name]
    hits = []
    for t in range(c.n_rounds):
        right, wrong = P.joint_reference(c, t, layout), P.joint_reference(c, t, layout, defect)
        if not (P.same_or_both_nan(right[0], wrong[0]) and P.same_or_both_nan(right[1], wrong[1])):
            hits.append(t)
    return hits


# defect -> (case, layout) that the defect turns red
JOINT_KILLERS = {
    "second_step_dropped": [("D260-k5-Nq3-query_onehot", "contiguous"), ("D1280-k1-Nq1-train_onehot", "contiguous"),
                            ("D16384-k9-Nq1-query_onehot", "contiguous")],
    "last_chunk_dropped": [("D256-k5-Nq1-train_onehot", "contiguous"), ("D1024-k5-Nq3-query_onehot", "contiguous")],
    "train_stride_is_D": [("D516-k127-Nq3-query_onehot", "window"), ("D256-k1-Nq1-train_onehot", "window"),
                          ("D16384-k9-Nq1-query_onehot", "window")],
    "query_stride_is_D": [("D516-k127-Nq3-query_onehot", "window"), ("D256-k1-Nq1-train_onehot", "window")],
    "query_row_0": [("D1028-k1-Nq3-train_onehot", "contiguous"), ("D1024-k128-Nq3-query_onehot", "window")],
    "tail_skipped": [("D260-k129-Nq1-query_onehot", "contiguous"), ("D256-k5-Nq1-train_onehot", "contiguous"),
                     ("D1024-k127-Nq3-query_onehot", "window")],
}


def test_every_joint_defect_has_a_killer():
    assert set(JOINT_KILLERS) == set(P.JS_DEFECTS)


@pytest.mark.parametrize("defect,name,layout", [(d, n, l) for d in JOINT_KILLERS for n, l in JOINT_KILLERS[d]])
def test_each_joint_defect_is_rejected_by_its_named_case(defect, name, layout):
    hits = _joint_differs(name, layout, defect)
    assert hits, (defect, name)
    c = JOINT[name]
    if defect == "second_step_dropped":                                         # exactly the rounds that pin a column of a later step
        assert hits == [t for t in range(c.n_rounds) if any(col >= 256 for col in c.round(t)[3])]
    if defect == "last_chunk_dropped":
        assert hits == [t for t in range(c.n_rounds) if any(col >= c.D - 256 for col in c.round(t)[3])]


def test_a_wrong_stride_is_invisible_on_contiguous_tables_and_defects_of_the_other_kernel_do_not_apply():
    assert not _joint_differs("D516-k127-Nq3-query_onehot", "contiguous", "train_stride_is_D")
    assert not _joint_differs("D516-k127-Nq3-query_onehot", "contiguous", "query_stride_is_D")
    assert not _joint_differs("D1024-k5-Nq3-query_onehot", "contiguous", "second_step_dropped")
    assert not _joint_differs("D260-k5-Nq3-query_onehot", "contiguous", "last_chunk_dropped")


# ================================================================================================ trie
MIXED = lambda V: [[0], [V - 1, 0], [V - 1, V - 1, 9], [5], [5, 0], [5, V - 1], [5, 9, 3], [7, 7, 6, 4, 8], [V - 2, 3]]


def test_trie_keep_is_the_definition_on_well_formed_tables():
    V = 1027
    seqs = MIXED(V)
    case = P.TrieCase("well_formed", P.trie_of_sets(seqs), [[[]]], V=V)
    P.assert_contained(case)
    rows = [[]] + [s[:n] for s in seqs for n in range(1, len(s) + 1)] + [s + [P.EOS] for s in seqs] + [s[:1] + [P.EOS] + s[1:] for s in seqs]
    rows += [[4], [5, 4], [P.EOS], [7, 7, 6, 5], [V - 1, V - 1, 9, 9]]
    for h in rows:
        assert np.array_equal(P.trie_keep(case, [h]), P.keep_by_definition(seqs, [h], V)), h
    for defect in ("no_clamps", "duplicate_kept_twice", "walk_last_duplicate", "int32_history"):      # no damage, no repeat, no wide id:
        assert np.array_equal(P.trie_keep(case, rows[:20], defect), P.trie_keep(case, rows[:20]))      # these defects change nothing here


def test_the_undamaged_small_cases_are_the_definition_too():
    for name in ("chain40", "wide_ids"):
        c = TRIE[name]
        for rows in c.calls:
            assert np.array_equal(P.trie_keep(c, rows), P.keep_by_definition([P.CHAIN[:7], P.CHAIN], rows, c.V))


@pytest.mark.parametrize("name", list(TRIE))
def test_every_trie_table_keeps_an_unguarded_kernel_inside_its_buffers(name):
    c = TRIE[name]
    P.assert_contained(c)
    t = c.table
    assert t.null_edges or (len(t.tok_buf) == t.n_edges + 2 * P.MARGIN and t.tok_off == P.MARGIN)
    assert (t.tok_buf >= 0).all() and (t.tok_buf < c.V).all() and P.EOS not in t.tok_buf.tolist()
    for rows in c.calls:                                                         # and no row is left without a column
        keep = P.trie_keep(c, rows)
        assert keep.any(1).all() and keep.shape == (len(rows), c.V)
        h = P.history_rows(c, rows)
        assert h.dtype == np.int64 and h.shape[1] == c.prompt_len + len(rows[0]) + 3


def test_trie_cases_are_what_their_names_say():
    only_eos = lambda keep: keep.sum(1).tolist() == [1] * len(keep) and keep[:, P.EOS].all()
    for e in (0, 1):
        c = TRIE[f"no_edges-end{e}"]
        assert c.table.n_edges == 0 and c.table.null_edges and c.table.arrays()[3].tolist() == [e]
        assert all(only_eos(P.trie_keep(c, rows)) for rows in c.calls)
    c = TRIE["chain40"]
    assert c.table.n_nodes == 41 and sorted(len(rows[0]) for rows in c.calls) == [0, 1, 7, 39, 40]
    k39, k40 = P.trie_keep(c, c.calls[3]), P.trie_keep(c, c.calls[4])
    assert np.flatnonzero(k39[0]).tolist() == [P.CHAIN[39]] and only_eos(k39[1:]) and only_eos(k40)
    assert c.calls[3][3][10] == P.EOS and c.calls[3][3][11:] == P.CHAIN[10:38] and c.calls[3][1][20] != P.CHAIN[20]
    assert np.flatnonzero(P.trie_keep(c, c.calls[2])[0]).tolist() == [P.EOS, P.CHAIN[7]]           # an end node with a child
    c = TRIE["wide_ids"]
    t = P.WIDE_T
    assert [h[0] for h in c.calls[0]] == [2 ** 32 + t, t - 2 ** 32, 2 ** 31 + t, -1, t]
    for rows in c.calls:
        keep = P.trie_keep(c, rows)
        assert only_eos(keep[:4]) and not only_eos(keep[4:])
    for n in (2048, 2049):
        c = TRIE[f"fan{n}"]
        begin, tok, node, end = c.table.arrays()
        ids = tok[begin[1]:begin[2]].tolist()
        assert len(ids) == n and ids == sorted(set(ids)) and ids[0] == 0 and ids[-1] == c.V - 1 == 6150 and P.EOS not in ids
        groups = np.zeros(c.V + 1, int)
        groups[ids] = 1
        per_group = groups.reshape(-1, 4).sum(1)
        assert (per_group == 4).sum() >= 300 and (per_group == 0).sum() >= 100 and ((per_group > 0) & (per_group < 4)).sum() >= 100
        keep = P.trie_keep(c, c.calls[1])
        assert np.flatnonzero(keep[0]).tolist() == ids and c.calls[1][0] == [5] and keep[1].sum() == 4 and only_eos(keep[2:])
    c = TRIE["duplicate"]
    begin, tok, node, end = c.table.arrays()
    assert tok[begin[0]:begin[1]].tolist() == [5, 9, 9, 12] and node[1] != node[2] and tok[begin[1]:begin[2]].tolist() == [8, 9, 9, 10]
    assert np.flatnonzero(P.trie_keep(c, [[]])[0]).tolist() == [5, 9, 12]
    assert np.flatnonzero(P.trie_keep(c, [[9]])[0]).tolist() == [20]                                # the first of the two edges
    assert np.flatnonzero(P.trie_keep(c, [[5]])[0]).tolist() == [8, 9, 10]
    for name, value in (("root_minus1", -1), ("root_n_nodes", 7)):
        c = TRIE[name]
        assert c.roots().tolist() == [value, 0, 1, 2] and c.table.n_nodes == 7
        for rows in c.calls:
            keep = P.trie_keep(c, rows)
            assert only_eos(keep[:1]) and not only_eos(keep[1:2])
    for name, value in (("child_node_minus1", -1), ("child_node_n_nodes", 7)):
        c = TRIE[name]
        assert c.table.arrays()[2][0] == value
        assert np.flatnonzero(P.trie_keep(c, [[], [], [], []])[0]).tolist() == [104, 108, 115]
        assert only_eos(P.trie_keep(c, c.calls[1])[:1]) and only_eos(P.trie_keep(c, c.calls[2])[:1])
    lists = lambda name: [np.flatnonzero(k).tolist() for k in P.trie_keep(TRIE[name], [[], [], [], []])]
    assert TRIE["begin_minus3"].table.arrays()[0].tolist() == [0, -3, 5, 6, 6, 6, 6, 6]
    assert lists("begin_minus3") == [[1], [104, 108, 115, 116, 123], [1, 142], [1]]                 # end < begin: empty; begin clamped to 0
    assert TRIE["begin_past_edges"].table.arrays()[0].tolist() == [0, 3, 11, 6, 6, 6, 6, 6]
    assert lists("begin_past_edges") == [[104, 108, 115], [116, 123, 142], [1], [1]]
    assert TRIE["begin_decreasing"].table.arrays()[0].tolist() == [0, 3, 1, 6, 6, 6, 6, 6]
    assert lists("begin_decreasing") == [[104, 108, 115], [1], [1, 108, 115, 116, 123, 142], [1]]
    c = TRIE["rows_per_item3"]
    assert c.rows_per_item == 3 and c.roots().tolist() == [0, -1, 2]
    sound = P.TrieCase("sound", c.table, c.calls, roots=[0, 0, 2], rows_per_item=3)
    for rows in c.calls:
        keep, other = P.trie_keep(c, rows), P.trie_keep(sound, rows)
        assert only_eos(keep[3:6]) and np.array_equal(keep[:3], other[:3]) and np.array_equal(keep[6:], other[6:]) and not only_eos(keep[:3])
    assert {c.name for c in TRIE.values() if c.damaged} == {"root_minus1", "root_n_nodes", "child_node_minus1", "child_node_n_nodes",
                                                           "begin_minus3", "begin_past_edges", "begin_decreasing", "rows_per_item3"}


# defect -> cases that the defect turns red
TRIE_KILLERS = {
    "int32_history": ["wide_ids"],
    "no_clamps": ["root_minus1", "root_n_nodes", "child_node_minus1", "child_node_n_nodes", "begin_minus3", "begin_past_edges",
                  "begin_decreasing", "rows_per_item3"],
    "is_end_at_leaf": ["no_edges-end0", "begin_minus3"],
    "duplicate_kept_twice": ["duplicate"],
    "walk_last_duplicate": ["duplicate"],
}


def test_every_trie_defect_has_a_killer():
    assert set(TRIE_KILLERS) == set(P.TRIE_DEFECTS)


@pytest.mark.parametrize("defect,name", [(d, n) for d in TRIE_KILLERS for n in TRIE_KILLERS[d]])
def test_each_trie_defect_is_rejected_by_its_named_case(defect, name):
    c = TRIE[name]
    assert any(not np.array_equal(P.trie_keep(c, rows), P.trie_keep(c, rows, defect)) for rows in c.calls), (defect, name)
    if defect == "int32_history":                                               # 2**32 + t and t - 2**32 wrap to t; 2**31 + t and -1 do not
        wrong = P.trie_keep(c, c.calls[0], defect)
        assert [bool(np.array_equal(wrong[r], wrong[4])) for r in range(4)] == [True, True, False, False]
