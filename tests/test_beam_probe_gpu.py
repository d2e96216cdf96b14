"""GPU: exact tie, edge and second-pass probes for ``eavqa_beam_step`` / ``eavqa_beam_step_logprobs`` / ``eavqa_beam_reorder``
(csrc/beam.hip).  Cases and references: tests/_select_probe.py (``ref_step`` of tests/test_beam_gpu.py; what each case is and that it
is not vacuous: tests/test_select_probe_cpu.py).  On the log-probability entry everything is ``torch.equal``, scores included, and the
row kernel's own 2k-lists are read back from the workspace; on the plain-logits entry the scores use ``_close`` (2e-5).  Every row
case runs on ``ld == V``, on a padded ``ld`` whose pad holds 1e30, and on a view 4 bytes off a 16-byte boundary (scalar loads).

Which case enters which path (and the mutation that turns it red; "run" = built into a scratch copy of the library and run on the
MI355X with the result stated; "read" = argued from the code):
  before(): the smaller column among equals   test_row_kernel_logprobs[tie_run-*], [all_equal-*], [minus_inf_*], [same_owner-* (k >= 3)],
                                              test_row_kernel_plain_logits[*], test_nan_*             `i < i2` -> `i > i2` in before() (run:
                                              every beam-step test of this file red - their rows of eighths tie often - except
                                              [same_owner-*-k1] and [tiny-V3-k1], which select no two equal values; the reorder tests green)
  owner rescan, several winners in a row      test_row_kernel_logprobs[same_owner-*]: one thread, chunks 4096 apart, ragged last chunk;
                                              a rescan of the first chunk alone loses the winners of the other chunks (read)
  rescan past the end of a short row          [minus_inf_short-*], [minus_inf_all-*], [tiny-*]: -inf columns by column, V = 2k, 2k + 1 (read)
  load4: vector / scalar / ragged tail        all of the above x (exact, padded, offset): a pad column read would win with 1e30 (read)
  merge: the earlier beam stays               test_merge[merge_tie-*], test_row_kernel_plain_logits[plain_cross_beam]
                                              `v > bvv` -> `v >= bvv` (read)
  merge: `r < k` with a tie at rank k - 1 / k test_merge[merge_tie-*-eos_first], [-eos_second], [plain_cross_beam]        (read)
  merge: next running beams, a hitter (+ -1e9) ranks above a candidate at -inf
                                              test_row_kernel_logprobs[minus_inf_short-k1], [minus_inf_all-*], [tiny-V2-k1] (run: the code
                                              before this file existed took "the candidates that did not hit first" and these five were red)
  pool: stable pick, open slot vs -1e9        test_cont_bits_and_the_tail_protocol[*]: an unfinished -1e9 slot ties with masked candidates (read)
  sequence gather beyond position 255         test_merge[long_sequences]                    `p += BM_THREADS` -> one pass only (run, together
                                              with the reorder mutation below: exactly the tests named in these two entries red)
  tail protocol: B = 1, B = 300, three items  test_merge[many_items-*], test_cont_bits_and_the_tail_protocol: the second step's flag is
                                              right only if the first left both sync words zeroed        (read)
  NaN ranks as -inf, never an index >= V      test_nan_*[nan_short-*] (run: the code before this file existed returned tokens of
                                              2147483647 in all six; [nan_scattered-*] were green then as now)
  beam_reorder_kernel beyond vector 255       test_reorder_long_rows[*], test_reorder_parent_out_of_range[*] (inner 2056),
                                              test_beam_gpu.py::test_beam_reorder_is_index_select[*-2056-*]     `c += 256` -> one pass only (run)
  beam_reorder_kernel parent out of range     test_reorder_parent_out_of_range: the row keeps its sentinel (read)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _select_probe as P
from test_beam_gpu import _close

DEV = "cuda"
PAD = 1.0e30


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


LAYOUTS = ("exact", "padded", "offset")


def layout(rows, name):
    """device view [R, V] of the rows: contiguous; inside a padded buffer full of 1e30; the same 4 bytes off a 16-byte boundary"""
    R, V = rows.shape
    if name == "exact":
        return rows.to(DEV)
    c0 = 0 if name == "padded" else 1
    buf = torch.full((R, (V + (32 if name == "padded" else 8) + 3) // 4 * 4), PAD)
    buf[:, c0:c0 + V] = rows
    view = buf.to(DEV)[:, c0:c0 + V]
    assert view.data_ptr() % 16 == 4 * c0 and view.stride(0) % 4 == 0 and view.stride(0) > V
    return view


def load_state(ops, case, st=None):
    st = ops.BeamState(case.B, case.k, case.max_length, 0, 1, DEV) if st is None else st
    b = case.before
    st.run_scores.copy_(b["run_scores"])
    st.run_seq.copy_(b["run_seq"].reshape(case.B * case.k, -1))
    st.pool_seq.copy_(b["pool_seq"].reshape(case.B * case.k, -1))
    st.pool_scores.copy_(b["pool_scores"])
    st.pool_len.copy_(b["pool_len"].to(torch.int32))
    st.pool_fin.copy_(b["pool_fin"].to(torch.int32))
    st.improve.copy_(b["improve"].to(torch.int32))
    return st


def workspace_lists(st):
    """the row kernel's candidates as the merge read them: (tokens int64 [R, 2k], values float32 [R, 2k])"""
    n = st.B * st.k * 2 * st.k
    val = st.ws[:4 * n].view(torch.float32).view(st.B * st.k, 2 * st.k).cpu()
    tok = st.ws[4 * n:8 * n].view(torch.int32).view(st.B * st.k, 2 * st.k).cpu().long()
    return tok, val


def check_step(st, case, want, cur_len, what, exact):
    B, k = case.B, case.k
    w = want["after"]
    assert torch.equal(st.next_tokens.cpu(), want["tokens"]), what
    assert torch.equal(st.parents.cpu().long(), want["parents"]), what
    assert torch.equal(st.run_seq.cpu().view(B, k, -1), w["run_seq"]), what
    assert torch.equal(st.pool_seq.cpu().view(B, k, -1), w["pool_seq"]), what
    assert torch.equal(st.pool_len.cpu().long(), w["pool_len"]), what
    assert torch.equal(st.pool_fin.cpu().bool(), w["pool_fin"]), what
    assert torch.equal(st.improve.cpu().bool(), w["improve"]), what
    assert int(st.cont[cur_len].item()) == int(want["cont"]), what
    if exact:
        assert torch.equal(st.run_scores.cpu(), w["run_scores"]), what
        assert torch.equal(st.pool_scores.cpu(), w["pool_scores"]), what
    else:
        _close(st.run_scores, w["run_scores"], what + " running scores")
        _close(st.pool_scores, w["pool_scores"], what + " pool scores")


def run_case(ops, case, every_layout):
    want = P.reference(case)
    for name in (LAYOUTS if every_layout else LAYOUTS[:1]):
        st = load_state(ops, case)
        for n, (s, w) in enumerate(zip(case.steps, want)):
            if s.get("reset"):
                load_state(ops, case, st)
            view = layout(s["rows"], name)
            st.cont.fill_(-1)
            ops.beam_step(view, case.V, st, s["cur_len"], s["eos"], case.lp, case.es, logprobs=case.logprobs)
            what = f"{case.name} {name} step {n}"
            if n == 0:
                tok, val = workspace_lists(st)
                wt, wv = P.row_lists(s["rows"], case.before["run_scores"], case.k)
                assert torch.equal(tok, wt), what
                if case.logprobs:
                    assert torch.equal(val, wv), what
            check_step(st, case, w, s["cur_len"], what, exact=case.logprobs)
            assert int(st.cont.ne(-1).sum()) == 1, what                       # one flag word written, none beside it


# ------------------------------------------------------------------------------------------------ row kernel
@pytest.mark.parametrize("case", P.row_cases(), ids=repr)
def test_row_kernel_logprobs(ops, case):
    run_case(ops, case, every_layout=True)


@pytest.mark.parametrize("case", P.plain_cases(), ids=repr)
def test_row_kernel_plain_logits(ops, case):
    run_case(ops, case, every_layout=True)


# ------------------------------------------------------------------------------------------------ merge and the tail protocol
@pytest.mark.parametrize("case", P.merge_cases(), ids=repr)
def test_merge(ops, case):
    run_case(ops, case, every_layout=False)


@pytest.mark.parametrize("case", P.cont_cases(), ids=repr)
def test_cont_bits_and_the_tail_protocol(ops, case):
    """The step's flag is the AND of three bits that here come from three different workgroups ("all": 1), or lack one bit everywhere
    (0); the second step on the same ``BeamState`` gives the reference's flag only if the first left the two sync words zeroed."""
    run_case(ops, case, every_layout=False)
    want = P.reference(case)
    assert want[0]["cont"] == (case.info["which"] == "all")


# ------------------------------------------------------------------------------------------------ never an index outside the row
def _index_property(tok, rows, V, what):
    assert ((tok >= 0) & (tok < V)).all(), (what, tok)
    assert all(len(set(r.tolist())) == r.numel() for r in tok), (what, tok)
    picked_nan = torch.isnan(torch.gather(rows, 1, tok))
    n_ok = (~torch.isnan(rows)).sum(1, keepdim=True)
    ranks = torch.arange(tok.shape[1])[None, :]
    assert torch.equal(picked_nan, ranks >= n_ok), what                       # no NaN column ahead of a non-NaN one, none before it must


@pytest.mark.parametrize("logprobs", [True, False], ids=["logprobs", "plain"])
@pytest.mark.parametrize("case,exact", P.nan_cases(), ids=[c.name for c, _ in P.nan_cases()])
def test_nan_never_an_index_outside_the_row(ops, case, exact, logprobs):
    """NaN entries rank as -inf for the selection (as the sampling pick treats them, tests/test_sample_gpu.py): every token of every
    row's 2k-list and of ``next_tokens`` lies in [0, V), the lists hold no column twice, and a NaN column is taken only once the other
    columns are used up.  With at least 2k other columns per row (``exact``) the lists are the reference's and, on the
    log-probability entry, so is the whole step.  Only integers and scores are read back; nothing is gathered with these tokens."""
    s = case.steps[0]
    for name in LAYOUTS:
        view = layout(s["rows"], name)
        st = load_state(ops, case)
        ops.beam_step(view, case.V, st, s["cur_len"], s["eos"], case.lp, case.es, logprobs=logprobs)
        what = f"{case.name} {name}"
        tok, val = workspace_lists(st)
        _index_property(tok, s["rows"], case.V, what)
        nt = st.next_tokens.cpu()
        assert ((nt >= 0) & (nt < case.V)).all(), (what, nt)
        assert ((st.run_seq.cpu() >= 0) & (st.run_seq.cpu() < case.V)).all(), what
        if exact:
            wt, wv = P.row_lists(s["rows"], case.before["run_scores"], case.k)
            assert torch.equal(tok, wt), what
            if logprobs:
                assert torch.equal(val, wv), what
                check_step(st, case, P.reference(case)[0], s["cur_len"], what, exact=True)


# ------------------------------------------------------------------------------------------------ K / V cache reorder
@pytest.mark.parametrize("dtype,inner", [(torch.bfloat16, 2056), (torch.bfloat16, 4096), (torch.float32, 1028)], ids=["bf16-257", "bf16-512", "f32-257"])
@pytest.mark.parametrize("t", [1, 3], ids=["t1", "t_max"])
def test_reorder_long_rows(ops, dtype, inner, t):
    """Rows of 257 and 512 16-byte vectors (the second pass of the copy loop), ``t == t_max`` included."""
    rows, t_max, planes = 5, 3, 2
    assert inner * (2 if dtype == torch.bfloat16 else 4) // 16 in (257, 512)
    g = torch.Generator().manual_seed(inner + t)
    src = torch.randn(planes, rows, t_max, inner, generator=g).to(dtype).to(DEV)
    keep = src.clone()
    for parents in ([4, 4, 0, 2, 2], [3, 0, 4, 1, 2]):
        dst = torch.full_like(src, 7.0)
        ops.beam_reorder(src, dst, torch.tensor(parents, dtype=torch.int32, device=DEV), t)
        assert torch.equal(dst[:, :, :t], src.index_select(1, torch.tensor(parents, device=DEV))[:, :, :t])
        assert (dst[:, :, t:] == 7.0).all() and torch.equal(src, keep)


@pytest.mark.parametrize("bad", [-1, 5])
def test_reorder_parent_out_of_range(ops, bad):
    """A parent outside [0, rows) never becomes an address: that destination row keeps its sentinel, the others are exact."""
    rows, t_max, planes, inner, t = 5, 4, 2, 2056, 3
    src = torch.randn(planes, rows, t_max, inner, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).to(DEV)
    keep = src.clone()
    parents = [2, 0, bad, 4, 1]
    dst = torch.full_like(src, 7.0)
    ops.beam_reorder(src, dst, torch.tensor(parents, dtype=torch.int32, device=DEV), t)
    good = [r for r in range(rows) if r != 2]
    want = src.index_select(1, torch.tensor([parents[r] for r in good], device=DEV))
    assert torch.equal(dst[:, good, :t], want[:, :, :t])
    assert (dst[:, 2] == 7.0).all() and (dst[:, :, t:] == 7.0).all() and torch.equal(src, keep)
