"""CPU: the cases of tests/_select_probe.py are what their names say, and none of them is vacuous - evaluating the reference with a
wrong tie rule (larger column wins, later beam wins, unstable pool pick), or without the second pass of a loop, changes what the
GPU tests expect."""
import numpy as np
import pytest
import torch

import _select_probe as P

ROW = {c.name: c for c in P.row_cases()}
PLAIN = {c.name: c for c in P.plain_cases()}
MERGE = {c.name: c for c in P.merge_cases()}
CONT = {c.name: c for c in P.cont_cases()}
NANS = {c.name: (c, exact) for c, exact in P.nan_cases()}
EXACT = {**ROW, **MERGE, **CONT}


# ================================================================================================ top-k
def test_topk_key_is_the_documented_order():
    x = np.concatenate([P.NEG_NAN[[1, 0, 2]], np.array([-np.inf, -3.4e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.4e38, np.inf], np.float32),
                        P.POS_NAN[[2, 0, 1]]])
    key = P.key_of(x).astype(np.int64)
    d = np.diff(key)
    assert (d[:7] > 0).all() and d[7] == 0 and (d[8:] > 0).all()           # ascending, the two zeros equal
    val, idx = P.topk_reference(x[None, ::-1].copy(), len(x))
    assert np.array_equal(idx[0], np.arange(len(x)))                       # the reversed row is already sorted: zeros in column order
    assert P.same_bits(val[0], x[::-1]).all() and not P.same_bits(P.POS_NAN[:1], P.POS_NAN[1:2]).any()
    assert P.same_bits(np.float32([0.0]), np.float32([-0.0])).all()


def test_topk_reference_is_numpy_on_ordinary_rows():
    x, _ = P.topk_cases()["grid_1025"]
    val, idx = P.topk_reference(x, 300)
    assert np.array_equal(idx, np.argsort(-x.astype(np.float64), axis=1, kind="stable")[:, :300])


def test_topk_grid_is_the_issues_grid():
    cases = P.topk_cases()
    for cols in (1, 2, 63, 64, 65, 1023, 1024, 1025):
        x, ks = cases[f"grid_{cols}"]
        assert x.shape[1] == cols and set(ks) == {1, cols}
    assert cases["grid_5000"][1] == (1025, 2047, 2048) and cases["grid_100003"][1] == (2048,)
    assert P.topk_seg(1) == 64 and P.topk_seg(1025) == 128 and P.topk_seg(100003) == 6272       # below a segment / a wave: 1 .. 65


def test_topk_tie_cut_lies_inside_a_later_segment():
    c = P.TIE_CUT
    x, (k,) = P.topk_cases()["tie_cut"]
    seg = P.topk_seg(c["cols"])
    for row in x:
        eq = np.flatnonzero(row == c["T"])
        assert (row > c["T"]).sum() == c["n_gt"] and k - c["n_gt"] == c["need_eq"] and list(eq) == c["eq_cols"]
        waves = eq // seg
        assert len(set(waves)) >= 3
        last = eq[c["need_eq"] - 1]                                         # the last element equal to T that is kept
        mine = eq[waves == last // seg]
        assert last // seg == sorted(set(waves))[1] and mine[0] < last < mine[-1]
    assert not np.array_equal(P.topk_reference(x, k)[1], P.topk_reference(x, k, larger_column_wins=True)[1])


def test_topk_low_byte_keys_differ_in_the_last_radix_byte_only():
    cases = P.topk_cases()
    for name, sign in (("low_byte", 1.0), ("low_byte_negated", -1.0)):
        x, ks = cases[name]
        for row in x:
            planted = row[(sign * row) >= 1.0]
            key = P.key_of(planted)
            assert len(planted) == 256 and len(set(key >> 8)) == 1 and len(set(key & 255)) == 256
            rest = row[(sign * row) < 1.0]
            assert (P.key_of(rest) >> 8 != key[0] >> 8).all()
            assert (rest < planted.min()).all() if sign > 0 else (rest > planted.max()).all()
        for k in ks:                                                        # the k-th key is one of the 256
            val, _ = P.topk_reference(x, k)
            assert (np.abs(val[:, -1]) >= 1.0).all()


def test_topk_bucket_zero_rows():
    cases = P.topk_cases()
    x, _ = cases["bucket0_huge_negative"]
    assert (x <= -2.0 ** 127).all() and (P.key_of(x) >> 24 == 0).all()      # first pass: every key in bucket 0
    x, ks = cases["bucket0_subnormals_zeros"]
    zero = P.key_of(np.float32([0.0]))[0]
    assert zero & 0x00FFFFFF == 0                                           # the zero key: bucket 0 in the three later passes
    assert ((x == 0).sum(1) == 200).all() and (np.signbit(x[x == 0])).sum() == 200 and (x <= 0).all()
    sub = x[x != 0]
    assert (np.abs(sub) < 2.0 ** -126).all() and (sub < 0).all()
    val, idx = P.topk_reference(x, 200)
    assert (val == 0).all() and (P.topk_reference(x, 201)[0][:, -1] < 0).all()
    assert np.array_equal(idx, np.stack([np.flatnonzero(r == 0) for r in x]))   # zeros of both signs tie: by column


def test_topk_special_value_rows():
    cases = P.topk_cases()
    x, ks = cases["minus_inf_fill"]
    for row, n in zip(x, (37, 1)):
        assert np.isfinite(row).sum() == n and max(ks) > n
        val, idx = P.topk_reference(row[None], 100)
        assert np.isfinite(val[0, :n]).all() and (val[0, n:] == -np.inf).all()
        assert np.array_equal(idx[0, n:], np.flatnonzero(row == -np.inf)[:100 - n])
    x, ks = cases["nans"]
    bits = x.view(np.uint32)
    assert sorted(bits[0][np.isnan(x[0])].tolist()) == sorted(np.concatenate([P.POS_NAN, P.NEG_NAN]).view(np.uint32).tolist())
    val, idx = P.topk_reference(x, x.shape[1])
    assert np.array_equal(val[0, :3].view(np.uint32), P.POS_NAN[[1, 0, 2]].view(np.uint32))       # payloads descending, then the finite
    assert np.array_equal(val[0, -3:].view(np.uint32), P.NEG_NAN[[2, 0, 1]].view(np.uint32))      # ..., then the negative NaNs
    assert np.isnan(val[:, :3]).all() and np.isnan(val[:, -3:]).all() and not np.isnan(val[0, 3:-3]).any()
    head = [c for c in idx[1, :9].tolist() if 700 <= c < 705]
    assert head == [700, 701, 702, 703, 704]                                # equal NaN keys: in column order


# ================================================================================================ beam: exactness
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_cases_meet_the_exactness_condition(name):
    """... and the float64 evaluation of the same case agrees with the float32 one wherever its result is representable."""
    case = EXACT[name]
    P.assert_exact_inputs(case)
    assert case.logprobs and (case.B * case.k <= 24 or name == "many_items-B300")
    r32, r64 = P.reference(case), P.reference(case, dtype=torch.float64)
    for a, b in zip(r32, r64):
        assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["parents"], b["parents"]) and a["cont"] == b["cont"]
        for n, v in a["after"].items():
            w = b["after"][n]
            if not v.is_floating_point():
                assert torch.equal(v, w), n
                continue
            ok = w.float().double() == w                                    # representable (a sentinel plus a score is not)
            assert torch.equal(v[ok].double(), w[ok]), n
            assert n != "run_scores" or ok[torch.isfinite(w) & (w > -1.0e8)].all()      # sums alone: always representable


# ================================================================================================ beam: row kernel
def _lists(case, **kw):
    s = case.steps[0]
    return P.row_lists(s["rows"], case.before["run_scores"], case.k, **kw)


@pytest.mark.parametrize("name", [n for n in sorted(ROW) if n.startswith("same_owner")])
def test_same_owner_cases(name):
    case = ROW[name]
    tok, _ = _lists(case)
    n = case.info["owned"]
    assert n >= 2 and (n == 2 * case.k or name == "same_owner-V4100-k8")
    for row in tok:
        owners = {P.row_thread(c) for c in row[:n].tolist()}
        assert len(owners) == 1                                             # one thread owns n consecutive winners
        assert n < 4 or (row[:n] >= 4096).any()                             # some of them beyond its first chunk
        assert row[:n].tolist() != sorted(row[:n].tolist())                 # not in column order
    dropped = case.steps[0]["rows"].clone()                                 # the owner's later chunks unread: another answer
    dropped[:, 4096:] = -P.INF
    assert n < 4 or not torch.equal(P.row_lists(dropped, case.before["run_scores"], case.k)[0], tok)
    assert case.V in (32128, 4100) and (case.V != 4100 or case.V % 4096 == 4)


@pytest.mark.parametrize("name", [n for n in sorted(ROW) if n.startswith("tie_run")])
def test_tie_run_cases(name):
    case = ROW[name]
    k = case.k
    tok, val = _lists(case)
    rows = case.steps[0]["rows"]
    for r, cols in enumerate(case.info["ties"]):
        assert len(cols) == 3 * k and len(set(cols)) == 3 * k and (rows[r, cols] == rows[r].max()).all() and (rows[r] == rows[r].max()).sum() == 3 * k
        assert tok[r].tolist() == cols[:2 * k]                              # the run straddles rank 2k
        kept, cut = cols[:2 * k], cols[2 * k:]
        assert any(P.row_thread(a) > P.row_thread(b) for a in kept for b in cut)        # a kept column in a later thread ...
        assert any(P.row_wave(a) > P.row_wave(b) for a in kept for b in cut)            # ... and in a later wave than a cut one
    assert not torch.equal(_lists(case, larger_column_wins=True)[0], tok)
    assert P.differs(P.reference(case), P.reference(case, rule="larger_column"))


def test_the_other_row_cases():
    for k in P.KS:
        tok, _ = _lists(ROW[f"all_equal-k{k}"])
        assert (tok == torch.arange(2 * k)).all()
        assert P.differs(P.reference(ROW[f"all_equal-k{k}"]), P.reference(ROW[f"all_equal-k{k}"], rule="larger_column"))
        case = ROW[f"minus_inf_short-k{k}"]
        rows = case.steps[0]["rows"]
        assert (torch.isfinite(rows).sum(1) == 2 * k - 1).all() and (case.V == 32128) == (k == 8)
        tok, val = _lists(case)
        assert torch.isfinite(val[:, :-1]).all() and (val[:, -1] == -P.INF).all()
        assert all(int(t) == int((rows[r] == -P.INF).nonzero()[0]) for r, t in enumerate(tok[:, -1]))
        if k == 1:                                                          # item 0: the eos candidate (+ -1e9) is kept, not the -inf one
            ref = P.reference(case)[0]
            assert int(ref["tokens"][0]) == case.steps[0]["eos"] and torch.isfinite(ref["after"]["run_scores"][0, 0])
        rows = ROW[f"minus_inf_one_beam-k{k}"].steps[0]["rows"]
        dead = (rows == -P.INF).all(1)
        assert dead.sum() == 2 and torch.isfinite(rows[~dead]).all() and (k == 1 or not dead.view(2, k).all(1).any())
        assert (ROW[f"minus_inf_all-k{k}"].steps[0]["rows"] == -P.INF).all()
        ref = P.reference(ROW[f"minus_inf_all-k{k}"])[0]
        assert ref["tokens"].tolist() == list(range(k)) * 2 and (ref["after"]["run_scores"] == -P.INF).all()
        assert ROW[f"tiny-V{2 * k}-k{k}"].V == 2 * k and ROW[f"tiny-V{2 * k + 1}-k{k}"].V == 2 * k + 1


# ================================================================================================ beam: plain logits
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_plain_logit_ties_are_bit_equal_and_everything_else_keeps_the_margin(name):
    case = PLAIN[name]
    k = case.k
    rows = case.steps[0]["rows"]
    levels = rows.unique()
    assert len(levels) <= 16 and (levels[1:] - levels[:-1]).min() >= 0.5
    gaps = P.plain_gaps(case)
    for g in gaps:
        assert (g == 0).any() and (g[g != 0] >= P.MARGIN).all()              # exact ties (bit-equal values) and nothing close otherwise
    if name == "plain_tie_run":
        assert all(g[2 * k - 1] == 0 for g in gaps)                         # ranks 2k - 1 and 2k are tied: the run is cut there
        for r, cols in case.info["ties"].items():
            assert len(cols) == 3 * k and (rows[r, cols] == rows[r].max()).all()
            assert any(P.row_thread(a) > P.row_thread(b) for a in cols[:k] for b in cols[-k:])
        assert P.differs(P.reference(case), P.reference(case, rule="larger_column"))
    else:
        assert torch.equal(rows[0], rows[1]) and torch.equal(rows[k], rows[k + 1])
        assert (case.before["run_scores"][:, 0] == case.before["run_scores"][:, 1]).all()
        assert gaps[0][k - 1] == 0 and gaps[1][2 * k - 1] == 0                # item 0: ranks k - 1 / k tied; item 1: ranks 2k - 1 / 2k
        ref = P.reference(case)[0]
        assert ref["after"]["pool_fin"][0].sum() == 1                       # of item 0's two tied eos candidates only rank k - 1 enters
        assert P.differs(P.reference(case), P.reference(case, rule="later_beam"))


# ================================================================================================ beam: merge
@pytest.mark.parametrize("name", [n for n in sorted(MERGE) if n.startswith("merge_tie")])
def test_merge_tie_cases(name):
    case = MERGE[name]
    k, plan, eos = case.k, case.info["plan"], case.steps[0]["eos"]
    s = case.steps[0]
    acc = (s["rows"].view(case.B, k, -1) + case.before["run_scores"][:, :, None]).reshape(case.B, -1)
    v, i = torch.sort(acc, dim=-1, descending=True, stable=True)
    for b in range(case.B):
        assert [(float(v[b, r]), int(i[b, r]) // case.V, int(i[b, r]) % case.V) for r in range(len(plan))] == [tuple(p) for p in plan]
    for hi in (k - 1, 2 * k - 1):                                           # tied across beams, the earlier beam holds the larger token
        (v0, b0, t0), (v1, b1, t1) = plan[hi], plan[hi + 1]
        assert v0 == v1 and b0 < b1 and t0 > t1
    ref = P.reference(case)[0]
    entered = ref["after"]["pool_fin"].sum(1)
    assert (entered == {-1: 0, plan[k - 1][2]: 1, plan[k][2]: 0}[eos]).all()
    assert P.differs(P.reference(case), P.reference(case, rule="later_beam"))


def test_long_sequences_case_takes_the_second_pass():
    case = MERGE["long_sequences"]
    assert case.max_length == 300 and case.k == 8 and [s["cur_len"] for s in case.steps] == [5, 270]
    ref = P.reference(case)
    flat = torch.arange(case.B * case.k)
    for step, cur in zip(ref, (5, 270)):
        assert not torch.equal(step["parents"], flat)                       # parents permuted
        assert (step["after"]["pool_len"] == cur + 1).any()                 # a hypothesis admitted at this length
        assert (step["after"]["pool_len"] == 4).any()                       # and an old one that stays
        for n in ("run_seq", "pool_seq"):                                   # positions 256 .. left as they were: another answer
            once = step["after"][n].clone()
            once[:, :, 256:] = step["before"][n][:, :, 256:]
            assert not torch.equal(once, step["after"][n]), n
    assert len(case.before["run_seq"].unique()) == case.B * case.k * 300    # every (row, position) holds its own value


def test_many_items_cases():
    for B in (1, 300):
        case = MERGE[f"many_items-B{B}"]
        assert case.B == B and case.k == 2 and case.V == 64 and len(case.steps) == 2
        ref = P.reference(case)
        assert ref[0]["cont"]                                               # the loop goes on: the second step is a real one
        assert B == 1 or any(not torch.equal(s["parents"], torch.arange(2 * B)) for s in ref)


@pytest.mark.parametrize("name", sorted(CONT))
def test_cont_cases_take_one_bit_each_from_a_different_item(name):
    case = CONT[name]
    which = case.info["which"]
    ref = P.reference(case)
    first = ref[0]
    improve = first["after"]["improve"]
    open_slot = ~first["after"]["pool_fin"].all(1)
    live = case.steps[0]["cur_len"] + 1 < case.max_length                   # below max_length every item has candidates that did not hit
    assert case.B == 3 and case.es is True and len(case.steps) == 2
    assert improve.tolist() == [which != "no_improve", False, False]
    assert open_slot.tolist() == [False, which != "no_open_slot", False]
    assert live == (which != "no_live_candidate")
    assert first["cont"] == (which == "all")
    if which == "all":                                                      # item 1: the open -1e9 slot ties with masked candidates
        assert P.differs(ref, P.reference(case, rule="unstable_pool"))


# ================================================================================================ beam: NaN rows
@pytest.mark.parametrize("name", sorted(NANS))
def test_nan_cases(name):
    case, exact = NANS[name]
    rows = case.steps[0]["rows"]
    n_ok = (~torch.isnan(rows)).sum(1)
    assert torch.isnan(rows).any(1).all()
    if exact:
        assert (n_ok >= 2 * case.k).all() and torch.isnan(rows[:, :4]).all()          # the smallest columns are NaN: never chosen
        tok, val = _lists(case)
        assert not torch.isnan(torch.gather(rows, 1, tok)).any() and torch.isfinite(val).all()
    else:
        assert (n_ok < 2 * case.k).all() and n_ok[-1] == 0                            # fewer than 2k usable columns; the last row has none
        assert case.k == 1 or set(n_ok.tolist()) == set(range(2 * case.k - 1))        # 0 .. 2k - 2 of them over the rows
