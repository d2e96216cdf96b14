"""Cases and references for the exact probes of the two selection families, importable without a GPU:
``eavqa_beam_step`` / ``eavqa_beam_step_logprobs`` (csrc/beam.hip) and ``eavqa_topk_rows`` (csrc/retrieval.hip).
tests/test_select_probe_cpu.py asserts that every case is what its name says and is not vacuous; tests/test_beam_probe_gpu.py and
tests/test_topk_probe_gpu.py run them on the device.

Top-k reference: a stable argsort on the kernel's documented key (``key_of`` in retrieval.hip): the order-preserving uint32 image of
the float with -0 equal to +0, a NaN with the sign bit clear above +inf, a NaN with the sign bit set below -inf; ties go to the
smaller column; values compare as bit patterns, both zeros allowed for +-0.

Beam reference: ``ref_step`` of tests/test_beam_gpu.py.  On the log-probability entry the rows reach it through ``reference``, which
hands them to ``ref_step`` in place of its ``log_softmax``.  Exactness condition of those cases (``assert_exact_inputs``): row
entries are multiples of 1/8 in [-64, 0] or -inf, running scores multiples of 1/8 in [-64, 0] or the -1e9 sentinel, length_penalty
in {0, 1, 2}: every sum is one IEEE addition, every division has an integer divisor and is correctly rounded on both sides, so the
scores are compared with ``torch.equal``.

Column ownership (from the code): in ``beam_row_kernel`` column c belongs to thread ``(c >> 2) & 1023`` of wave ``thread >> 6``; in
``topk_rows_kernel`` wave w owns columns ``[w * seg, (w + 1) * seg)`` with ``seg = roundup64(ceil(cols / 16))``."""
import contextlib
import functools
import math

import numpy as np
import torch

import test_beam_gpu as tb
from test_beam_gpu import MARGIN, NEG, Gaps, _top, init_state, ref_step  # noqa: F401  (re-exported to the probe tests)

INF = math.inf
NAN = math.nan


# ================================================================================================ top-k
def key_of(x):
    """uint32 keys of float32 values, ascending in the kernel's order."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where((u & 0x80000000) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def topk_reference(x, k, larger_column_wins=False):
    """(values float32 [rows, k], columns int64 [rows, k]) of the k largest keys per row, ties by the smaller column
    (``larger_column_wins``: the wrong rule, for the vacuity checks)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    inv = (~key_of(x)).astype(np.int64)                      # ascending in this = descending in the key
    if larger_column_wins:
        idx = x.shape[1] - 1 - np.argsort(inv[:, ::-1], axis=1, kind="stable")[:, :k]
    else:
        idx = np.argsort(inv, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(x, idx, 1), idx.astype(np.int64)


def same_bits(got, want):
    """Elementwise: the same bit pattern, or both a zero of either sign."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))


def topk_seg(cols):
    return ((cols + 15) // 16 + 63) // 64 * 64


def f32_bits(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


POS_NAN = f32_bits([0x7FC00000, 0x7FC00001, 0x7F800001])     # sign clear: above +inf, ordered by payload
NEG_NAN = f32_bits([0xFFC00000, 0xFFC00001, 0xFF800001])     # sign set: below -inf, the larger payload further down

TIE_CUT = dict(cols=3000, T=1.0, n_gt=40, eq_cols=[384 + 5, 384 + 70, 384 + 130, 576 + 3, 576 + 64, 576 + 100, 576 + 191, 768 + 7, 768 + 90],
               need_eq=5)                                    # seg = 192: three equal in wave 2, four in wave 3, two in wave 4
LOW_BYTE_KS = (1, 100, 255, 256)
LOW_BYTE_FILL = 300


def _grid_rows(r, cols):
    x = r.standard_normal((3, cols)).astype(np.float32)
    x[1] = np.round(x[1] * 4) / 4                            # heavy ties, zeros of both signs
    x[1, cols // 3] = -0.0
    x[2, : max(1, cols // 2)] = x[2, 0]                      # one long run of ties from column 0
    return x


@functools.lru_cache(maxsize=None)
def topk_cases():
    """name -> (float32 [rows, cols], tuple of k)"""
    cases = {}
    r = np.random.RandomState(20)
    for cols in (1, 2, 63, 64, 65, 1023, 1024, 1025):
        cases[f"grid_{cols}"] = (_grid_rows(r, cols), tuple(sorted({1, cols})))
    cases["grid_5000"] = (_grid_rows(r, 5000), (1025, 2047, 2048))
    cases["grid_100003"] = (_grid_rows(r, 100003), (2048,))

    c = TIE_CUT
    x = (r.rand(2, c["cols"]) * 0.9).astype(np.float32)
    free = np.setdiff1d(np.arange(c["cols"]), c["eq_cols"])
    for row in range(2):
        x[row, c["eq_cols"]] = c["T"]
        x[row, r.permutation(free)[: c["n_gt"]]] = (2.0 + r.rand(c["n_gt"])).astype(np.float32)
    cases["tie_cut"] = (x, (c["n_gt"] + c["need_eq"],))

    vals = (1.0 + np.arange(256) * 2.0 ** -23).astype(np.float32)
    x = (r.rand(2, 2000) * 0.9).astype(np.float32)
    for row in range(2):
        x[row, r.permutation(2000)[:256]] = vals[r.permutation(256)]
    cases["low_byte"] = (x, LOW_BYTE_KS)
    cols = 256 + LOW_BYTE_FILL
    x = (r.rand(2, cols) * 0.9).astype(np.float32)             # the larger filler: all of it ranks first
    for row in range(2):
        x[row, r.permutation(cols)[:256]] = -vals[r.permutation(256)]
    cases["low_byte_negated"] = (x, tuple(LOW_BYTE_FILL + k for k in LOW_BYTE_KS))

    x = -(1.8e38 + r.rand(2, 700) * 1.5e38).astype(np.float32)
    x[1, 100:400] = x[1, 100]
    cases["bucket0_huge_negative"] = (x, (1, 350, 700))
    x = -f32_bits(r.randint(1, 1 << 23, (2, 700)))             # negative subnormals ...
    zeros = r.permutation(700)[:200]
    x[:, zeros[:100]] = 0.0                                    # ... and zeros of both signs
    x[:, zeros[100:]] = -0.0
    cases["bucket0_subnormals_zeros"] = (x.astype(np.float32), (1, 150, 200, 201, 700))

    cases["all_equal"] = (np.full((2, 3000), -2.5, np.float32), (1, 1000, 2048))
    cases["all_minus_inf"] = (np.full((2, 3000), -INF, np.float32), (1, 1000, 2048))
    x = r.standard_normal((2, 3000)).astype(np.float32)
    x[0, 2222] = INF
    x[1, 0] = INF
    cases["one_plus_inf"] = (x, (1, 2, 2048))
    x = np.full((2, 3000), -INF, np.float32)
    for row, n in enumerate((37, 1)):
        x[row, r.permutation(3000)[:n]] = r.standard_normal(n).astype(np.float32)
    cases["minus_inf_fill"] = (x, (1, 38, 100, 2048))
    x = r.standard_normal((2, 1500)).astype(np.float32)
    for row in range(2):
        at = r.permutation(1500)[:6]
        x[row, at[:3]] = POS_NAN[r.permutation(3)]
        x[row, at[3:]] = NEG_NAN[r.permutation(3)]
    x[1, 700:705] = POS_NAN[0]                                 # equal NaN keys: by column
    cases["nans"] = (x, (1, 3, 5, 1500))
    return cases


# ================================================================================================ beam step
def row_thread(c):
    return (int(c) >> 2) & 1023


def row_wave(c):
    return row_thread(c) >> 6


class Case:
    """One beam-search state and the steps taken from it.  ``steps``: dicts(rows float32 [B * k, V], cur_len, eos[, reset])."""

    def __init__(self, name, B, k, V, steps, before, max_length=8, lp=1.0, es=False, logprobs=True, exact_rows=True, **info):
        self.name, self.B, self.k, self.V, self.steps, self.before = name, B, k, V, steps, before
        self.max_length, self.lp, self.es, self.logprobs, self.exact_rows, self.info = max_length, lp, es, logprobs, exact_rows, info

    def __repr__(self):
        return self.name


def eighths(g, shape, lo, hi):
    """multiples of 1/8 in [lo, hi)"""
    return torch.randint(int(lo * 8), int(hi * 8), shape, generator=g).to(torch.float32) / 8


def state(B, k, max_length, run_scores=None):
    st = init_state(B, k, max_length, 0, 1)
    if run_scores is not None:
        st["run_scores"] = run_scores.clone().to(torch.float32).reshape(B, k)
    return st


def assert_exact_inputs(case):
    assert case.lp in (0.0, 1.0, 2.0)
    for what, x in [("rows", s["rows"]) for s in case.steps] + [("scores", case.before["run_scores"])]:
        fin = x[torch.isfinite(x) & (x > -1.0e8)]
        assert torch.equal(fin * 8, (fin * 8).round()) and (fin >= -64).all() and (fin <= 0).all(), (case.name, what)
        rest = x[~(torch.isfinite(x) & (x > -1.0e8))]
        assert ((rest == -INF) | (rest == NEG)).all() and (what == "scores" or (rest == -INF).all()), (case.name, what)


def _tie_order(x, n, group, key):
    """descending x, equal values by ``key`` ascending ((group, column) pairs; numpy lexsort, last key first)"""
    v = x.numpy()
    idx = np.arange(v.shape[-1])
    out = np.stack([np.lexsort(key(idx // group, idx % group) + (-row.astype(np.float64),)) for row in v])[:, :n]
    i = torch.from_numpy(out)
    return torch.take_along_dim(x, i, -1), i


WRONG_RULES = ("larger_column", "later_beam", "unstable_pool")


@contextlib.contextmanager
def _patched(V, rule, rows_as_logprobs):
    """``ref_step`` with (a) its log_softmax replaced by the given rows (the log-probability entry: the rows ARE the log-probabilities)
    and (b) one of its three selections made with a wrong tie rule.  Both are put back on exit."""
    calls = [0]

    def top(x, n, gaps):
        calls[0] += 1
        which = (calls[0] - 1) % 3                           # ref_step: candidates [B, k * V], next beams [B, 2k], pool [B, 3k]
        if rule == "larger_column" and which == 0:
            return _tie_order(x, n, V, lambda beam, col: (-col, beam))
        if rule == "later_beam" and which == 0:
            return _tie_order(x, n, V, lambda beam, col: (col, -beam))
        if rule == "unstable_pool" and which == 2:
            return _tie_order(x, n, x.shape[-1], lambda grp, e: (-e,))
        return _top(x, n, gaps)

    keep_top, keep_ls = tb._top, torch.log_softmax
    tb._top = top
    if rows_as_logprobs is not None:
        torch.log_softmax = lambda x, dim=-1: rows_as_logprobs
    try:
        yield
    finally:
        tb._top, torch.log_softmax = keep_top, keep_ls


def nan_as_minus_inf(rows):
    return torch.where(torch.isnan(rows), torch.tensor(-INF), rows)


def reference(case, rule=None, dtype=torch.float32):
    """Per step: dict(before, after, tokens, parents, cont) from ``ref_step``.  NaN entries rank as -inf.  ``dtype=torch.float64``:
    the same evaluation with every score in float64."""
    st = {n: (v.to(dtype) if v.is_floating_point() else v).clone() for n, v in case.before.items()}
    out, gaps = [], Gaps()
    fresh = lambda: {n: (v.to(dtype) if v.is_floating_point() else v).clone() for n, v in case.before.items()}
    for s in case.steps:
        if s.get("reset"):                                   # the case's first state again (in the same device buffers)
            st = fresh()
        rows = nan_as_minus_inf(s["rows"]).to(dtype)
        with _patched(case.V, rule, rows if case.logprobs else None):
            after, tokens, parents, cont = ref_step(st, rows, case.V, case.k, s["cur_len"], case.max_length, s["eos"], case.lp, case.es, gaps)
        out.append(dict(before=st, after=after, tokens=tokens, parents=parents, cont=cont))
        st = after
    return out


def row_lists(rows, run_scores, k, larger_column_wins=False):
    """What ``beam_row_kernel`` leaves per decoder row on the log-probability entry: (tokens int64 [R, 2k], values float32 [R, 2k]),
    descending value, ties by the smaller column, NaN as -inf, value + the row's running score."""
    x = nan_as_minus_inf(rows)
    if larger_column_wins:
        v, i = torch.sort(x.flip(-1), dim=-1, descending=True, stable=True)
        i = x.shape[-1] - 1 - i
    else:
        v, i = torch.sort(x, dim=-1, descending=True, stable=True)
    return i[:, :2 * k], v[:, :2 * k] + run_scores.reshape(-1, 1).to(torch.float32)


def differs(a, b):
    """two ``reference`` results differ in something the GPU test compares"""
    for x, y in zip(a, b):
        if not (torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["parents"], y["parents"]) and x["cont"] == y["cont"]):
            return True
        if any(not torch.equal(x["after"][n], y["after"][n]) for n in x["after"]):
            return True
    return False


# ------------------------------------------------------------------------------------------------ row kernel, log-probability entry
KS = (1, 3, 8)
TIE_FIXED = [8, 4000, 28672]          # threads 2, 1000 (wave 15) and 0: the largest column, always cut, belongs to the first thread
TIE_POOL = [256, 300, 1000, 2049, 4096, 4097, 4104, 4352, 5000, 8192, 8200, 9000, 12544, 13000, 16384, 16388, 17001, 20000, 20480, 21002,
            24576, 24580, 25003]


def _base(seed, B, k, V):
    g = torch.Generator().manual_seed(seed)
    return g, eighths(g, (B * k, V), -64, -32), eighths(g, (B, k), -4, 0.125)


def _one_step(name, B, k, V, rows, run, cur_len=2, eos=-1, **kw):
    kw.setdefault("max_length", 8)
    return Case(name, B, k, V, [dict(rows=rows, cur_len=cur_len, eos=eos)], state(B, k, kw["max_length"], run), **kw)


def same_owner_columns(V, row):
    """the columns of ONE thread, in column order: V = 32128: 16 columns, 4 of one float4 in each of 4 chunks 4096 apart;
    V = 4100: thread 0's 8 columns, 4 of them in the ragged last chunk"""
    if V == 4100:
        return [0, 1, 2, 3, 4096, 4097, 4098, 4099]
    t = 5 + 37 * row
    return [4 * t + j + 4096 * m for m in range(4) for j in range(4)]


@functools.lru_cache(maxsize=None)
def row_cases():
    cases = []
    for k in KS:
        B = 2
        R = B * k
        for V in (32128, 4100):                              # the largest values sit in columns of one thread
            g, rows, run = _base(100 + k + V, B, k, V)
            for r in range(R):
                own = same_owner_columns(V, r)
                n = min(2 * k, len(own))
                at = [own[i] for i in torch.randperm(len(own), generator=g)[:n].tolist()]
                if at == sorted(at):
                    at.reverse()
                rows[r, at] = -torch.arange(n, dtype=torch.float32) / 8 - 1       # distinct, in a scrambled column order ...
                if n >= 4:
                    rows[r, at[3]] = rows[r, at[2]]                               # ... and one equal pair inside the thread
                if n < 2 * k:                                                      # (V = 4100, k = 8: ranks 8 .. 15 lie elsewhere)
                    rest = (torch.randperm(V - 8, generator=g)[:2 * k - n] + 4).tolist()
                    rows[r, rest] = -torch.arange(2 * k - n, dtype=torch.float32) / 8 - 8
            cases.append(_one_step(f"same_owner-V{V}-k{k}", B, k, V, rows, run, eos=22, owned=min(2 * k, len(same_owner_columns(V, 0)))))

        V = 32128                                            # 3k equal maxima, the smaller column in a later thread / wave
        g, rows, run = _base(200 + k, B, k, V)
        ties = []
        for r in range(R):
            extra = [TIE_POOL[i] for i in torch.randperm(len(TIE_POOL), generator=g)[:3 * k - 3].tolist()]
            cols = sorted(TIE_FIXED + extra)
            rows[r, cols] = -1.0
            ties.append(cols)
        cases.append(_one_step(f"tie_run-k{k}", B, k, V, rows, run, ties=ties))

        V = 4100
        g, rows, run = _base(300 + k, B, k, V)
        rows[:] = -2.0
        cases.append(_one_step(f"all_equal-k{k}", B, k, V, rows, run))

        V = 32128 if k == 8 else 4100                        # exactly 2k - 1 finite entries
        g, rows, run = _base(400 + k, B, k, V)
        rows[:] = -INF
        for r in range(R):
            at = torch.randperm(V, generator=g)[:2 * k - 1]
            rows[r, at] = eighths(g, (2 * k - 1,), -8, 0.125)
        # eos = the best token of row 0: a candidate that hit (+ -1e9) ranks above the -inf ones among the next running beams
        cases.append(_one_step(f"minus_inf_short-k{k}", B, k, V, rows, run, eos=int(rows[0].argmax())))
        V = 4100                                             # one beam's row all -inf
        g, rows, run = _base(500 + k, B, k, V)
        rows[:, torch.randperm(V, generator=g)[:40]] = eighths(g, (R, 40), -8, 0.125)
        rows[k - 1] = -INF
        rows[k] = -INF
        cases.append(_one_step(f"minus_inf_one_beam-k{k}", B, k, V, rows, run))
        g, rows, run = _base(600 + k, B, k, V)
        rows[:] = -INF
        cases.append(_one_step(f"minus_inf_all-k{k}", B, k, V, rows, run, eos=0))

        for V in (2 * k, 2 * k + 1):                         # every column (but one) is selected
            g, rows, run = _base(700 + k + V, B, k, V)
            rows = eighths(g, (R, V), -3, 0.125)
            rows[0, 0] = -INF
            cases.append(_one_step(f"tiny-V{V}-k{k}", B, k, V, rows, run, eos=1))
    return cases


# ------------------------------------------------------------------------------------------------ row kernel, plain logits
@functools.lru_cache(maxsize=None)
def plain_cases():
    """Rows of a few levels at least 0.5 apart: equal logits give bit-equal log-probabilities on both sides."""
    B, k, V = 2, 3, 4100
    g = torch.Generator().manual_seed(31)
    filler = lambda: -3.0 - 0.5 * torch.randint(0, 7, (B * k, V), generator=g).to(torch.float32)
    # a tie run inside a row: item 0 takes its first step (beams 1.. at -1e9), beam 0 holds 3k equal maxima; item 1: beam 1's run of
    # 3k starts below beam 0's k maxima and is cut at rank 2k
    rows = filler()
    t0, t1 = [8, 256, 300, 1000, 2048, 4096, 4097, 4098, 4099], [3, 8, 256, 700, 2049, 3000, 4096, 4098, 4099]
    rows[0, t0] = 2.0
    rows[3, [5, 300, 4097]] = 2.0
    rows[4, t1] = 2.0
    run = torch.tensor([[0.0, NEG, NEG], [-0.5, -1.0, -9.0]])
    within = _one_step("plain_tie_run", B, k, V, rows, run, cur_len=1, logprobs=False, exact_rows=False, ties={0: t0, 4: t1})
    # cross-beam: beams 0 and 1 of an item hold the same row at equal running scores
    rows = filler()
    top = [4097, 300, 8, 2048, 1000]
    for item in range(B):
        rows[item * k, top] = torch.tensor([3.0, 2.5, 2.0, 1.5, 1.0])
        rows[item * k + 1] = rows[item * k]
    rows[5, 77] = 4.0                                        # item 1's beam 2 puts one candidate ahead of the pairs
    run = torch.tensor([[-0.5, -0.5, NEG], [-1.0, -1.0, -1.25]])
    cross = _one_step("plain_cross_beam", B, k, V, rows, run, cur_len=1, logprobs=False, exact_rows=False, eos=300)
    return [within, cross]


def plain_gaps(case):
    """Per item the differences between adjacent values of the top 2k + 1 accumulated log-probabilities (sentinels left out) - with a
    first step, an empty pool and length_penalty 1 every later selection ranks a subset of the same values."""
    s = case.steps[0]
    acc = torch.log_softmax(s["rows"], -1).view(case.B, case.k, case.V) + case.before["run_scores"][:, :, None]
    v = torch.sort(acc.reshape(case.B, -1), dim=-1, descending=True, stable=True)[0][:, :2 * case.k + 1]
    return [(row[:-1] - row[1:])[(row[1:] > -1.0e8)] for row in v]


# ------------------------------------------------------------------------------------------------ merge
def _planted(g, B, k, V, plan, run):
    """rows whose item-wide ranking starts with ``plan``: a list of (value, beam, token), descending; everything else is far below"""
    rows = eighths(g, (B * k, V), -64, -40)
    for b in range(B):
        for value, beam, token in plan:
            rows[b * k + beam, token] = value - float(run[b, beam])
    return rows


def merge_tie_plan(k):
    """ranks k - 1 / k tied between beams 0 and k - 1, ranks 2k - 1 / 2k between beams 1 and k - 1; the earlier beam holds the LARGER
    token, so a rule on the token alone fails too"""
    plan = []
    for r in range(2 * k + 2):
        plan.append([-3.0 - r, (r * 5 + 2) % k, 20 + r])
    plan[k - 1][1:], plan[k][1:] = [0, 19], [k - 1, 4]
    plan[k][0] = plan[k - 1][0]
    plan[2 * k - 1][1:], plan[2 * k][1:] = [1, 17], [k - 1, 3]
    plan[2 * k][0] = plan[2 * k - 1][0]
    return [tuple(p) for p in plan]


@functools.lru_cache(maxsize=None)
def merge_cases():
    cases = []
    V = 64
    for k in (3, 8):
        B = 2
        g = torch.Generator().manual_seed(40 + k)
        run = eighths(g, (B, k), -2, 0.125)
        plan = merge_tie_plan(k)
        rows = _planted(g, B, k, V, plan, run)
        for tag, eos in (("none", -1), ("first", 19), ("second", 4)):     # eos: nobody / the rank k - 1 candidate / the rank k candidate
            cases.append(_one_step(f"merge_tie-k{k}-eos_{tag}", B, k, V, rows, run, cur_len=3, eos=eos, lp=2.0, plan=plan))

    # max_length 300: the sequence gather's second pass (positions 256 ..), steps at cur_len 5 and 270
    B, k, L = 2, 8, 300
    g = torch.Generator().manual_seed(50)
    st = state(B, k, L, eighths(g, (B, k), -4, 0.125))
    pos = torch.arange(L)[None, None, :]
    st["run_seq"] = (1000 * torch.arange(B * k).view(B, k, 1) + pos).clone()
    st["pool_seq"] = (500000 + 1000 * torch.arange(B * k).view(B, k, 1) + pos).clone()
    st["pool_scores"][:, :3] = torch.tensor([-0.5, -1.0, -1.5])         # three finished hypotheses that stay, five open slots
    st["pool_fin"][:, :3] = True
    st["pool_len"][:, :3] = 4
    steps = [dict(rows=eighths(g, (B * k, V), -6, 0.125), cur_len=c, eos=e) for c, e in ((5, 11), (270, 12))]
    for s in steps:
        s["rows"][::2, s["eos"]] = 0.0                        # every other beam ends here: hypotheses enter the pool at both lengths
    cases.append(Case("long_sequences", B, k, V, steps, st, max_length=L, lp=0.0, es=False))

    for B in (1, 300):                                       # one merge workgroup; more merge (300) and row (600) workgroups than CUs
        k = 2
        g = torch.Generator().manual_seed(60 + B)
        steps = [dict(rows=eighths(g, (B * k, V), -4, 0.125), cur_len=c, eos=7) for c in (1, 2)]
        st = state(B, k, 8)
        st["improve"][(B + 1) // 2:] = False
        cases.append(Case(f"many_items-B{B}", B, k, V, steps, st, max_length=8, lp=1.0, es=True))
    return cases


CONT_BITS = ("all", "no_improve", "no_open_slot", "no_live_candidate")


@functools.lru_cache(maxsize=None)
def cont_cases():
    """B = 3, early_stopping=True.  "all": item 0 is the only one whose improvement flag stays up, item 1 the only one with an open
    pool slot, and every item has candidates that did not hit: the three bits meet only in the last workgroup's OR.  (The third bit
    cannot come from one item alone: an item's 2k candidates hold at most k eos tokens, one per beam, so below max_length every item
    sets it, and at max_length none does.)  The other three cases take one bit away everywhere.  Each case is two steps on one set of
    device buffers; after the step at max_length - 1 every running score carries -1e9, where float32 sums no longer tell candidates
    apart, so that case's second step starts from the first state again (``reset``)."""
    B, k, V, L = 3, 2, 64, 8
    cases = []
    for which in CONT_BITS:
        g = torch.Generator().manual_seed(70)
        st = state(B, k, L, eighths(g, (B, k), -2, 0.125))
        st["improve"] = torch.tensor([which != "no_improve", False, False])
        st["pool_fin"][:] = True
        st["pool_scores"][:] = -5.0e8                        # finished with scores that even a beam ended by -1e9 / length improves on
        st["pool_len"][:] = 2
        if which != "no_open_slot":
            st["pool_fin"][1, 1] = False
            st["pool_scores"][1, 1] = NEG
            st["pool_len"][1, 1] = 1
        c0 = L - 1 if which == "no_live_candidate" else 3
        steps = [dict(rows=eighths(g, (B * k, V), -4, 0.125), cur_len=c, eos=9) for c in ((c0,) if c0 == L - 1 else (c0, c0 + 1))]
        if c0 == L - 1:                                      # the step at max_length - 1 ends every beam: the second one starts over
            steps.append(dict(rows=eighths(g, (B * k, V), -4, 0.125), cur_len=c0, eos=9, reset=True))
        cases.append(Case(f"cont-{which}", B, k, V, steps, st, max_length=L, lp=1.0, es=True, which=which))
    return cases


# ------------------------------------------------------------------------------------------------ NaN rows
@functools.lru_cache(maxsize=None)
def nan_cases():
    """(case, exact): ``exact`` = every row keeps at least 2k non-NaN columns, so NaN columns are never chosen and the rest is exact."""
    out = []
    for k in (1, 3, 8):
        B, V = 2, 4100
        R = B * k
        g, rows, run = _base(800 + k, B, k, V)
        rows[:, torch.randperm(V, generator=g)[:60]] = eighths(g, (R, 60), -8, 0.125)
        for r in range(R):
            rows[r, torch.randperm(V, generator=g)[:500]] = NAN
        rows[:, :4] = NAN
        out.append((_one_step(f"nan_scattered-k{k}", B, k, V, rows, run), True))
        g, rows, run = _base(900 + k, B, k, V)
        rows[:] = NAN
        for r in range(R - 1):                               # 0 .. 2k - 1 non-NaN columns; the last row is all NaN
            n = r % (2 * k)
            rows[r, torch.randperm(V, generator=g)[:n]] = eighths(g, (n,), -8, 0.125)
        out.append((_one_step(f"nan_short-k{k}", B, k, V, rows, run), False))
    return out
