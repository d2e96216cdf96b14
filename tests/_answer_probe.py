"""Cases and references for the exact probes of the two kernels next to ``eavqa_topk_rows`` on the example-selection and the
answer-selection path, importable without a GPU: ``eavqa_rices_joint_scores`` (csrc/retrieval.hip, ``joint_scores_kernel<NC>``) and
``eavqa_trie_constrain`` (csrc/constrain.hip).  tests/test_answer_probe_cpu.py asserts that every case is what its name says and that
none is vacuous; tests/test_rices_probe_gpu.py and tests/test_trie_probe_gpu.py run them on the device through ctypes.

Joint scores.  Every table entry is a small integer and every text similarity a multiple of 1/2, so each sum is exact in float32 in
any order (``assert_joint_exact``) and results are compared with ``array_equal``.  A case is a shape (D, k, Nq) and a probe kind; it
is run in ROUNDS (``JointCase.round``) because one launch pins only a few columns, and over its rounds every column of
``probe_columns(D)`` is pinned:
  query_onehot   query image row q is 1 at column cols[q] and 0 elsewhere, the train rows are dense
                 (``train[v, c] = ((7 v + 13 c) mod 251) - 125``): ``img_sim[i, j] == train[q2img[text_idx[i, j]], c_q]`` - ONE element
                 of ONE gathered row.  Round t hands query i the one-hot row ``(t Nq + i) mod len(cols)``.
  train_onehot   the query rows are dense (``((11 q + 17 c) mod 241) - 120``, 121 in place of 0), train row v is ``v + 1`` at column
                 ``c_v`` and 0 elsewhere: this pins the LDS staging of the query row and the ``qv[]`` registers.  The first
                 ``step = min(k, Ni)`` neighbours of query 0 are train rows 3 .. 3 + step - 1 (mod Ni; never row 0 alone, whose
                 address does not depend on the stride), and round t puts ``c_v = cols[(t step + v) mod len(cols)]``.
Both kinds run in two layouts: ``contiguous`` and ``window`` (train rows ``D + 4`` apart, query rows ``D + 12`` apart; the pad columns
and one surplus row hold 3e4, so a read outside a row moves every sum it enters).

Trie.  ``trie_keep`` is a plain restatement of the contract of ``eavqa_trie_constrain`` in include/eavqa.h on RAW CSR arrays, with the
clamps exactly as the kernel's comment states them: ``begin = clamp(child_begin[n], 0, n_edges)``, ``end = clamp(child_begin[n + 1],
begin, n_edges)``, a root or a child node outside ``[0, n_nodes)`` = the row is off the trie and only eos is allowed.  It returns the
boolean keep mask.  Every table is a WINDOW inside a larger buffer whose surroundings hold filler that keeps any index within the
buffers (``assert_contained``): a kernel without a guard would compute other values, it could not leave the allocations.

The cases, by name (``trie_cases()``; V = 1027 in rows of 1032 floats unless stated, eos = 1, one prompt id in front of the history):
  no_edges-end0 / -end1     n_edges = 0 with child_tok = child_node = NULL, is_end[0] = 0 / 1: every row keeps eos alone ("a node
                            without children allows eos whatever is_end says").
  chain40                   41 nodes in a row; histories of 0, 1, 7 (an end node with a child), 39 and 40 ids (the leaf); a wrong id
                            at position 20 of 39 and of 40; eos in the middle with the true continuation behind it (the row stays
                            ended): "deep walks".
  wide_ids                  (the chain's table) history ids 2**32 + t, t - 2**32, 2**31 + t and -1 for a real child t are off the trie,
                            the row that holds t itself is on it, at the first and at the second id: "a history id is compared as
                            int64".
  fan2048 / fan2049         V = 6151.  A node REACHED BY A ONE-ID WALK whose child list holds 2048 (searched in LDS) / 2049 (searched
                            in global memory) ids, among them column 0 and column V - 1, with aligned groups of 4 columns entirely
                            full (8 .. 1207) and entirely empty (4000 .. 4399).
  duplicate                 the root's child list is [5, 9, 9, 12], the two 9s pointing at different nodes: the mask is that of
                            {5, 9, 12}, and a walk over 9 follows the FIRST of the two edges - the lower bound of the binary search,
                            as the code does; the contract says "distinct", so this pins what the code does with a list that is not.
                            The node behind 5 lists [8, 9, 9, 10]: the id behind the repeated one in the same group of 4 columns.
  root_minus1 / root_n_nodes                  roots[0] is -1 / n_nodes: that row keeps eos alone, the other rows are unaffected.
  child_node_minus1 / child_node_n_nodes      the edge the walk follows leads to -1 / n_nodes: off the trie from there on.
  begin_minus3 / begin_past_edges / begin_decreasing
                            child_begin[1] = -3, child_begin[2] = n_edges + 5, child_begin[2] < child_begin[1]: the lists the
                            restated clamps give (an empty one where end < begin).
  rows_per_item3            roots with rows_per_item = 3, the middle item's root damaged: its three rows keep eos alone, the six rows
                            of the other items are unaffected.
"""
import bisect
import functools
import math

import numpy as np

import _constrained_ref as cref

# ================================================================================================ joint scores
JS_BLOCK = 128                                    # neighbours of one query per workgroup (retrieval.hip)
JS_UNROLLED = {256: 1, 512: 2, 768: 3, 1024: 4}   # D -> NC of joint_scores_kernel<NC>; every other D runs <0>
JS_KS = (1, 5, 127, 128, 129)
JS_NQS = (1, 3)
JS_KINDS = ("query_onehot", "train_onehot")
JS_LAYOUTS = ("contiguous", "window")
JS_SHAPES = [(D, k) for D in (256, 260, 516, 1024, 1028, 1280) for k in JS_KS] + [(16384, 9)]
JS_PAD = 3.0e4
NI_DENSE, NI_ONEHOT, NQI_DENSE = 37, 40, 5
JS_DEFECTS = ("second_step_dropped", "last_chunk_dropped", "train_stride_is_D", "query_stride_is_D", "query_row_0", "tail_skipped")


def js_nc(D):
    return JS_UNROLLED.get(D, 0)


def js_rj(D):
    """neighbours a wave resolves at a time"""
    return 4 if js_nc(D) else 8


def probe_columns(D):
    """0, 3, 4, 252, 255, 256, 259, every multiple of 256 below D with the column before it, and the last four columns"""
    cols = {0, 3, 4, 252, 255, 256, 259} | set(range(D - 4, D))
    for m in range(256, D, 256):
        cols |= {m - 1, m}
    return sorted(c for c in cols if 0 <= c < D)


def dense_train(Ni, D):
    v, c = np.arange(Ni)[:, None], np.arange(D)[None, :]
    return ((7 * v + 13 * c) % 251 - 125).astype(np.float32)


def dense_query(Nqi, D):
    q, c = np.arange(Nqi)[:, None], np.arange(D)[None, :]
    x = (11 * q + 17 * c) % 241 - 120
    return np.where(x == 0, 121, x).astype(np.float32)        # no zero: a query column that is lost always shows


def window(table, ld):
    """[rows + 1, ld] full of 3e4 with the table in its first rows and columns (ld = D: the surplus row alone)"""
    rows, D = table.shape
    buf = np.full((rows + 1, ld), JS_PAD, np.float32)
    buf[:rows, :D] = table
    return buf


def js_lds(D, layout):
    """(ld_train, ld_query)"""
    return (D, D) if layout == "contiguous" else (D + 4, D + 12)


class JointCase:
    def __init__(self, D, k, Nq, kind):
        self.D, self.k, self.Nq, self.kind = D, k, Nq, kind
        self.name = f"D{D}-k{k}-Nq{Nq}-{kind}"
        self.cols = probe_columns(D)
        if kind == "query_onehot":
            self.Ni, self.Nqi = NI_DENSE, len(self.cols)
            self.n_rounds = -(-len(self.cols) // Nq)
            self._train = dense_train(self.Ni, D)
            self._query = np.zeros((self.Nqi, D), np.float32)
            self._query[np.arange(self.Nqi), self.cols] = 1.0
        else:
            self.Ni, self.Nqi = NI_ONEHOT, NQI_DENSE
            self.step = min(k, self.Ni)
            self.n_rounds = -(-len(self.cols) // self.step)
            self._query = dense_query(self.Nqi, D)
        self.Ndq = 3 * self.Ni + 5
        i, j = np.arange(Nq)[:, None], np.arange(k)[None, :]
        # neighbour j of query i is train question Ndq - 1 - u with u = (j + 11 i + 3) mod Ndq, whose image is row u mod Ni
        self.text_idx = ((self.Ndq - 1 - j - 11 * i - 3) % self.Ndq).astype(np.int64)
        self.q2img = ((self.Ndq - 1 - np.arange(self.Ndq)) % self.Ni).astype(np.int32)
        self.text_sim = (((3 * i + 5 * j) % 129 - 64) / 2).astype(np.float32)

    def __repr__(self):
        return self.name

    def image_rows(self):
        """train image row of every (query, neighbour)"""
        return self.q2img[self.text_idx]

    def round(self, t):
        """(train [Ni, D], query [Nqi, D], query_row int32 [Nq], the columns this round pins)"""
        n = len(self.cols)
        if self.kind == "query_onehot":
            rows = np.array([(t * self.Nq + i) % n for i in range(self.Nq)], np.int32)
            return self._train, self._query, rows, [self.cols[r] for r in rows]
        at = [self.cols[(t * self.step + v) % n] for v in range(self.Ni)]
        train = np.zeros((self.Ni, self.D), np.float32)
        train[np.arange(self.Ni), at] = np.arange(1, self.Ni + 1)
        rows = np.array([(2 * i + 1) % self.Nqi for i in range(self.Nq)], np.int32)
        reached = sorted(set(self.image_rows()[0].tolist()))
        return train, self._query, rows, [at[v] for v in reached]


@functools.lru_cache(maxsize=None)
def joint_cases():
    return [JointCase(D, k, Nq, kind) for D, k in JS_SHAPES for Nq in JS_NQS for kind in JS_KINDS]


@functools.lru_cache(maxsize=None)
def joint_case(name):
    return {c.name: c for c in joint_cases()}[name]


def assert_joint_exact(case, train, query):
    """integers, and the sum of |products| of any (query row, train row) plus the text similarity stays below 2^23 halves"""
    assert np.array_equal(train, np.round(train)) and np.array_equal(query, np.round(query)), case.name
    assert np.array_equal(case.text_sim * 2, np.round(case.text_sim * 2)) and np.abs(case.text_sim).max() <= 64, case.name
    largest = (np.abs(query.astype(np.float64)) @ np.abs(train.astype(np.float64)).T).max()
    assert largest + 64 < 2 ** 23, (case.name, largest)
    assert case.D * 125 < 2 ** 24                              # the bound of a dense row against a 0 / 1 row


def joint_reference(case, t, layout, defect=None, bufs=None):
    """float64 (joint, img_sim) [Nq, k] of round ``t``, evaluated on the flat buffers of ``layout`` so that a wrong stride reads what
    the kernel would read.  NaN = never written.  ``defect``: one of ``JS_DEFECTS`` (the vacuity checks).  ``bufs``: the round's
    (train, query) ``window`` buffers when the caller holds them already."""
    train, query, query_row, _ = case.round(t)
    D, k, Nq = case.D, case.k, case.Nq
    ld_t, ld_q = js_lds(D, layout)
    tbuf, qbuf = (window(train, ld_t), window(query, ld_q)) if bufs is None else bufs
    tbuf, qbuf = tbuf.reshape(-1), qbuf.reshape(-1)
    if defect == "train_stride_is_D":
        ld_t = D
    if defect == "query_stride_is_D":
        ld_q = D
    live = np.ones(D)
    if defect == "second_step_dropped" and js_nc(D) == 0:     # the generic kernel's column loop taken once
        live[256:] = 0
    if defect == "last_chunk_dropped" and js_nc(D) > 0:       # `s < NC - 1` in the unrolled kernels
        live[D - 256:] = 0
    rows = np.zeros_like(query_row) if defect == "query_row_0" else query_row
    Q = np.stack([qbuf[int(r) * ld_q:int(r) * ld_q + D] for r in rows]).astype(np.float64) * live
    T = np.stack([tbuf[v * ld_t:v * ld_t + D] for v in range(case.Ni)]).astype(np.float64)
    img = np.take_along_axis(Q @ T.T, case.image_rows().astype(np.int64), 1)
    joint = case.text_sim.astype(np.float64) + img
    if defect == "tail_skipped":                              # the last k % RJ neighbours keep the buffer's NaN
        cut = k - k % js_rj(D)
        joint[:, cut:] = math.nan
        img[:, cut:] = math.nan
    return joint, img


def same_or_both_nan(a, b):
    return bool(np.array_equal(a, b, equal_nan=True))


# ================================================================================================ trie
EOS = 1
MARGIN = 16
TRIE_DEFECTS = ("int32_history", "no_clamps", "is_end_at_leaf", "duplicate_kept_twice", "walk_last_duplicate")
TOK_PRE = np.arange(20, 20 + MARGIN)                          # ascending and below every id of the damaged tables
TOK_POST = np.arange(900, 900 + MARGIN)


class Table:
    """Raw CSR arrays as windows: ``x_buf[x_off : x_off + len]`` is array x, the rest of ``x_buf`` is filler."""

    def __init__(self, begin, tok, node, end, null_edges=False):
        self.n_nodes, self.n_edges, self.null_edges = len(end), len(tok), null_edges
        assert len(begin) == self.n_nodes + 1 and len(node) == self.n_edges
        live = not null_edges                                  # filler an unguarded kernel would act on (and still stay inside)
        self.cb_buf = np.concatenate([np.full(MARGIN, -2 if live else 0), begin, np.full(MARGIN, self.n_edges + 3 if live else 0)]).astype(np.int32)
        self.tok_buf = np.concatenate([TOK_PRE, tok, TOK_POST]).astype(np.int32)
        self.node_buf = np.concatenate([np.arange(MARGIN) % self.n_nodes, node, np.arange(MARGIN) % self.n_nodes]).astype(np.int32)
        self.end_buf = np.concatenate([np.ones(MARGIN), end, np.ones(MARGIN)]).astype(np.uint8)
        self.cb_off = self.tok_off = self.node_off = self.end_off = MARGIN

    def arrays(self):
        """(child_begin, child_tok, child_node, is_end) without their surroundings"""
        o = MARGIN
        return (self.cb_buf[o:o + self.n_nodes + 1], self.tok_buf[o:o + self.n_edges], self.node_buf[o:o + self.n_edges],
                self.end_buf[o:o + self.n_nodes])


def csr(children, end):
    """``children``: per node a list of (id, node), in the order given"""
    begin, tok, node = [0], [], []
    for ch in children:
        for t, n in ch:
            tok.append(t)
            node.append(n)
        begin.append(len(tok))
    return begin, tok, node, list(end)


class TrieCase:
    """``calls``: lists of histories (the generated ids of every row), one list per launch, all of one length."""

    def __init__(self, name, table, calls, V=1027, ld=1032, roots=None, rows_per_item=1, damaged=False):
        self.name, self.table, self.calls, self.V, self.ld, self.rows_per_item, self.damaged = name, table, calls, V, ld, rows_per_item, damaged
        self.prompt_len = 1
        self.roots_buf = None if roots is None else np.concatenate([np.zeros(MARGIN), roots, np.zeros(MARGIN)]).astype(np.int32)
        self.roots_off = MARGIN
        for rows in calls:
            assert len({len(h) for h in rows}) == 1 and len(rows) % rows_per_item == 0
            assert roots is None or len(rows) == len(roots) * rows_per_item

    def __repr__(self):
        return self.name

    def roots(self):
        return None if self.roots_buf is None else self.roots_buf[MARGIN:-MARGIN]


def _wrap32(t):
    return (int(t) + 2 ** 31) % 2 ** 32 - 2 ** 31


def trie_keep(case, rows, defect=None):
    """bool [R, V]: the columns ``eavqa_trie_constrain`` leaves finite for the histories ``rows``.  The arrays are read through their
    windows' offsets, so the variant without the guards (``no_clamps``) reads the filler a kernel without them would read."""
    t = case.table
    guard = defect != "no_clamps"
    cb = lambda i: int(t.cb_buf[t.cb_off + i])
    tk = lambda e: int(t.tok_buf[t.tok_off + e])
    nd = lambda e: int(t.node_buf[t.node_off + e])
    is_end = lambda n: int(t.end_buf[t.end_off + n])
    inside = lambda n: not guard or 0 <= n < t.n_nodes

    def children(n):
        b, e = cb(n), cb(n + 1)
        if guard:
            b = min(max(b, 0), t.n_edges)
            e = min(max(e, b), t.n_edges)
        return b, e

    keep = np.zeros((len(rows), case.V), bool)
    for r, hist in enumerate(rows):
        node = 0 if case.roots_buf is None else int(case.roots_buf[case.roots_off + r // case.rows_per_item])
        on = inside(node)
        begin, end = children(node) if on else (0, 0)
        for tok in hist:
            if not on:
                break
            tok = _wrap32(tok) if defect == "int32_history" else int(tok)
            lo, hi = begin, end
            while lo < hi:                                     # the lower bound
                mid = (lo + hi) >> 1
                if tk(mid) < tok:
                    lo = mid + 1
                else:
                    hi = mid
            if defect == "walk_last_duplicate":
                while lo + 1 < end and tk(lo + 1) == tok:
                    lo += 1
            on = lo < end and tk(lo) == tok
            if on:
                node = nd(lo)
                on = inside(node)
            if on:
                begin, end = children(node)
        n = end - begin if on else 0
        if defect == "is_end_at_leaf":
            eos_ok = not on or is_end(node) != 0
        else:
            eos_ok = not on or n == 0 or is_end(node) != 0
        ids = [tk(begin + i) for i in range(max(n, 0))]
        if defect == "duplicate_kept_twice":                   # the merge over 4 columns without the skip of a repeated id
            for c0 in range(0, case.V, 4):
                lo = bisect.bisect_left(ids, c0)
                for c in range(c0, min(c0 + 4, case.V)):
                    if lo < len(ids) and ids[lo] < c:
                        lo += 1
                    keep[r, c] = lo < len(ids) and ids[lo] == c
        else:
            for c in ids:
                if 0 <= c < case.V:
                    keep[r, c] = True
        if eos_ok:
            keep[r, EOS] = True
    return keep


def assert_contained(case):
    """Whatever value of the buffers an unguarded kernel took for an index - a child_begin entry (window or filler) as an edge index,
    a child_node / roots entry as a node index - the element it names, window offset added, lies inside the buffer."""
    t = case.table
    if t.null_edges:
        assert not t.cb_buf.any() and case.roots_buf is None     # no edge is ever named: nothing to follow
        return
    for b in t.cb_buf.tolist():
        assert 0 <= t.tok_off + b <= len(t.tok_buf) and 0 <= t.node_off + b <= len(t.node_buf), (case.name, b)
    nodes = t.node_buf.tolist() + ([] if case.roots_buf is None else case.roots_buf.tolist())
    for n in nodes:
        assert 0 <= t.cb_off + n and t.cb_off + n + 1 < len(t.cb_buf) and 0 <= t.end_off + n < len(t.end_buf), (case.name, n)


def trie_of_sets(sequences):
    """The table ``AnswerTrie`` builds for one set, as a :class:`Table` (well formed): for the check against tests/_constrained_ref.py."""
    kids, end = [dict()], [0]
    for s in sequences:
        node = 0
        for tok in s:
            if tok not in kids[node]:
                kids[node][tok] = len(kids)
                kids.append(dict())
                end.append(0)
            node = kids[node][tok]
        end[node] = 1
    return Table(*csr([[(tok, ch[tok]) for tok in sorted(ch)] for ch in kids], end))


def keep_by_definition(sequences, rows, V):
    """``_constrained_ref.walk`` as a keep mask"""
    keep = np.zeros((len(rows), V), bool)
    for r, h in enumerate(rows):
        keep[r, cref.walk(sequences, h, EOS)] = True
    return keep


CHAIN = [10 + 25 * i for i in range(40)]
WIDE_T, WIDE_T2 = CHAIN[0], CHAIN[1]
FAN_V = 6151
FAN_FULL, FAN_EMPTY = range(8, 8 + 4 * 300), range(4000, 4400)


def fan_ids(n):
    ids = {0, FAN_V - 1} | set(FAN_FULL)
    for t in np.random.RandomState(n).permutation(FAN_V).tolist():
        if len(ids) == n:
            break
        if t != EOS and t not in FAN_EMPTY:
            ids.add(t)
    return sorted(ids)


def _small(damage=None):
    """7 nodes, 6 edges with ids ascending over the WHOLE edge array (so that a list cut differently is still sorted):
    0: 104 -> 1, 108 -> 2, 115 -> 3;  1: 116 -> 4, 123 -> 5;  2: 142 -> 6;  3 .. 6: leaves (5 with is_end = 0)."""
    begin, tok, node, end = csr([[(104, 1), (108, 2), (115, 3)], [(116, 4), (123, 5)], [(142, 6)], [], [], [], []], [0, 0, 1, 1, 1, 0, 1])
    n_nodes, n_edges = 7, 6
    if damage == "child_node_minus1":
        node[0] = -1
    elif damage == "child_node_n_nodes":
        node[0] = n_nodes
    elif damage == "begin_minus3":
        begin[1] = -3
    elif damage == "begin_past_edges":
        begin[2] = n_edges + 5
    elif damage == "begin_decreasing":
        begin[2] = 1
    return Table(begin, tok, node, end)


SMALL_CALLS = [[[], [], [], []], [[104], [116], [142], [104]], [[104, 116], [116, 5], [142, 7], [104, 123]]]


@functools.lru_cache(maxsize=None)
def trie_cases():
    cases = []
    for e in (0, 1):
        cases.append(TrieCase(f"no_edges-end{e}", Table([0, 0], [], [], [e], null_edges=True), [[[], []], [[5], [EOS]], [[5, 9], [7, EOS]]]))

    table = Table(*csr([[(CHAIN[i], i + 1)] for i in range(40)] + [[]], [1 if i in (7, 40) else 0 for i in range(41)]))
    wrong = lambda n: CHAIN[:20] + [CHAIN[20] + 1] + CHAIN[21:n]
    cases.append(TrieCase("chain40", table, [
        [[]], [CHAIN[:1], [CHAIN[0] + 1]], [CHAIN[:7], CHAIN[:6] + [CHAIN[7]]],
        [CHAIN[:39], wrong(39), CHAIN[:10] + [EOS] + CHAIN[11:39], CHAIN[:10] + [EOS] + CHAIN[10:38]],
        [CHAIN[:40], wrong(40), CHAIN[:39] + [EOS]]]))

    t, t2 = WIDE_T, WIDE_T2
    cases.append(TrieCase("wide_ids", table, [                 # the chain's table: the row that stays on it shows at both depths
        [[2 ** 32 + t], [t - 2 ** 32], [2 ** 31 + t], [-1], [t]],
        [[t, 2 ** 32 + t2], [t, t2 - 2 ** 32], [t, 2 ** 31 + t2], [t, -1], [t, t2]]]))

    for n in (2048, 2049):
        ids = fan_ids(n)
        small = [0, 77, FAN_V - 1]
        table = Table(*csr([[(5, 1), (6, 2)], [(c, 3) for c in ids], [(c, 3) for c in small], []], [0, 0, 1, 1]))
        miss = next(c for c in range(2000, FAN_V) if c not in ids)
        cases.append(TrieCase(f"fan{n}", table, [[[]], [[5], [6], [7]], [[5, 0], [5, FAN_V - 1], [5, miss], [6, 77]]], V=FAN_V, ld=FAN_V + 1))

    table = Table(*csr([[(5, 1), (9, 2), (9, 3), (12, 4)], [(8, 5), (9, 5), (9, 5), (10, 5)], [(20, 5)], [(30, 5)], [], []], [0, 0, 0, 0, 1, 1]))
    cases.append(TrieCase("duplicate", table, [[[]], [[5], [9], [12], [10]], [[9, 20], [9, 30], [5, 9], [5, 10]]]))

    for damage in ("root_minus1", "root_n_nodes"):
        roots = [-1 if damage == "root_minus1" else 7, 0, 1, 2]
        calls = [[[], [], [], []], [[104], [104], [116], [142]]]
        cases.append(TrieCase(damage, _small(), calls, roots=roots, damaged=True))
    for damage in ("child_node_minus1", "child_node_n_nodes", "begin_minus3", "begin_past_edges", "begin_decreasing"):
        cases.append(TrieCase(damage, _small(damage), SMALL_CALLS, roots=[0, 1, 2, 3], damaged=True))
    rows = [[104], [108], [33], [104], [116], [EOS], [142], [104], [142]]
    cases.append(TrieCase("rows_per_item3", _small(), [[[]] * 9, rows], roots=[0, -1, 2], rows_per_item=3, damaged=True))
    return cases


@functools.lru_cache(maxsize=None)
def trie_case(name):
    return {c.name: c for c in trie_cases()}[name]


def history_rows(case, rows):
    """int64 [R, prompt_len + L + 3]: the prompt's ids are 0, the ids behind cur_len (never read) are 77"""
    L = len(rows[0])
    h = np.full((len(rows), case.prompt_len + L + 3), 77, np.int64)
    h[:, :case.prompt_len] = 0
    for r, ids in enumerate(rows):
        h[r, case.prompt_len:case.prompt_len + L] = ids
    return h
