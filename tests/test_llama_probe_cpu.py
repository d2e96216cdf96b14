"""No GPU: the probes of tests/_llama_probe.py are what they claim to be.  The rope data is exact (every expected value survives a round
trip through bfloat16), the tables cover the routes, strides and edges they name, the multi-pass cases are three passes with a ragged
tail and no pass boundary on a row boundary, the plain emulations of the kernels are accepted on every case, and every one-line mutation
of them is rejected by the case named here - so the acceptance functions tests/test_llama_probe_gpu.py uses can tell a kernel with that
defect from a correct one."""
import functools
import math

import pytest
import torch

import _llama_probe as P


@functools.lru_cache(maxsize=None)
def _rope_reference(name):
    c = P.BY_NAME[name]
    return P.reference_rope(c, P.materialize_rope(c)[1])


def run(c, mutation=None):
    """One case through its emulation and its acceptance function (AssertionError: rejected)."""
    if isinstance(c, P.RopeCase):
        win, v = P.materialize_rope(c)
        P.emulate_rope(c, win, v, mutation)
        P.check_rope(c, _rope_reference(c.name), *win["x"])
    elif isinstance(c, P.FinishCase):
        win, v = P.materialize_finish(c)
        want = P.reference_finish(c, v)
        P.emulate_finish(c, win, v, mutation)
        P.check_rope(c, want, *win["out"], what="out")
    else:
        win, v = P.materialize_swiglu(c)
        ref = P.reference_swiglu(c, v)
        P.emulate_swiglu(c, win, mutation)
        P.check_swiglu(c, ref, *win["out"])


# ------------------------------------------------------------------------------------------------------------------ the data is exact
def _quarters_in_bf16(x, lim):
    return bool(torch.equal(x * 4, (x * 4).round()) and x.abs().max().item() <= lim and torch.equal(x.to(torch.bfloat16).double(), x))


def test_rope_data_is_exact_and_survives_bfloat16():
    """The argument of the module docstring, checked value by value: tables in quarters within [-1, 1] and different from each other, x
    integers within 8, every expected value a multiple of 1/4 within 16 that bfloat16 holds exactly - and no expected value is the sentinel."""
    cos, sin = P.table_values(P.N_POS, 128)
    for t in (cos, sin):
        assert _quarters_in_bf16(t, 1.0)
    assert not torch.equal(cos, sin) and not torch.equal(cos[1:], cos[:-1]) and not torch.equal(cos[:, 1:], cos[:, :-1])
    for c in P.ROPE_CASES:
        v = P.materialize_rope(c)[1]
        want = _rope_reference(c.name)
        assert torch.equal(v["x"], v["x"].round()) and v["x"].abs().max().item() <= 8, c.name
        assert _quarters_in_bf16(want, 16.0), c.name
        assert not (want == P.SENTINEL).any()
    for c in P.FINISH_CASES:
        v = P.materialize_finish(c)[1]
        assert v["part"].abs().max().item() <= 2 and v["part"].sum(0).abs().max().item() <= 8, c.name
        for s in range(1, c.ks):
            assert not torch.equal(v["part"][s], v["part"][s - 1]), c.name
        assert _quarters_in_bf16(P.reference_finish(c, v), 16.0), c.name


def test_swiglu_data_is_exact_in_bfloat16_and_the_partial_sums_add_up():
    for c in P.SWIGLU_CASES:
        if c.multipass and c.dtype == "f32":
            continue
        win, v = P.materialize_swiglu(c)
        for nm in ("g", "b", "d"):
            assert torch.equal(v[nm].to(P.DT[c.dtype]).double(), v[nm]), (c.name, nm)          # (the edge gates: rounded to the case's type)
            assert c.edge or torch.equal(v[nm].to(torch.bfloat16).double(), v[nm]), (c.name, nm)
        assert bool(v["g"].isfinite().all())
        if not c.edge:
            assert v["g"].abs().max().item() <= 30 and v["b"].abs().max().item() <= 2 and v["d"].abs().max().item() <= 1
        if c.kind == "splitk":
            acc = torch.zeros(c.rows, 2 * c.F)
            for s in range(c.ks):                                                       # float32, slice order: as the kernel adds
                acc = acc + win["part"][1].view(c.ks, c.rows, 2 * c.F)[s]
            assert torch.equal(acc.double(), torch.cat([v["g"], v["b"]], dim=1)), c.name
    z = torch.tensor(-P.SILU_GRAD_ZERO, dtype=torch.float64)
    s = torch.sigmoid(z)
    assert abs((s * (1 + z * (1 - s))).item()) < 1e-15
    g = set(P.edge_gates("f32").tolist())
    assert {0.0, 16.0, -16.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max} <= g
    assert any(math.copysign(1.0, x) < 0 and x == 0 for x in P.edge_gates("bf16").tolist())          # -0 is there
    assert torch.finfo(torch.bfloat16).max in P.edge_gates("bf16").tolist()


# ------------------------------------------------------------------------------------------------------------- what the tables cover
def test_rope_cases_cover_every_route_stride_direction_and_position_edge():
    small = [c for c in P.ROPE_CASES if not c.multipass]
    for dtype, hds in P.ROPE_HD.items():
        for hd in hds:
            mine = [c for c in small if (c.dtype, c.hd) == (dtype, hd)]
            assert {(c.H, c.rows) for c in mine} == {(H, r) for H in (1, 3, 6) for r in (1, 5, 67)}
            assert {(c.table_cols, c.ld_table) for c in mine} == {(hd // 2, hd // 2), (hd // 2, hd // 2 + 4), (hd, hd)}
            assert {c.inverse for c in mine} == {False, True}
            assert all(c.ldx > c.H * c.hd for c in mine)
    assert {c.route for c in small} == {"f32-vec4", "bf16-vec8", "bf16-vec4"}
    assert {c.per_head for c in small if c.route == "bf16-vec4"} == {1, 3, 5}           # hd 8, 24, 40
    assert {c.pos_kind for c in small if c.rows == 1} == {"last", "zero", "below", "above"}
    p = P.positions(67, "mixed").tolist()
    assert p[0] == P.N_POS - 1 and p[1] == 0 and p[2] < 0 and p[3] == P.N_POS and p[5] == P.INT_MIN and p[6] == P.INT_MAX
    assert p[4] == p[7] and any(a > b for a, b in zip(p[8:], p[9:])) and len(set(p)) < len(p)        # repeated, non-monotonic
    assert P.positions(5, "mixed").tolist()[:4] == p[:4]                                             # five rows meet both sides too


def test_multipass_cases_are_three_ragged_passes_with_no_boundary_on_a_row():
    rope = [c for c in P.ROPE_CASES if c.multipass]
    assert sorted((c.route, c.per_head) for c in rope) == [("bf16-vec4", 3), ("bf16-vec8", 1), ("f32-vec4", 1)]
    for c in rope:
        assert P.multipass_violations(c.items, c.per_row) == [], c.name
        assert len(list(P._passes(c.items, None))) == 3
        assert (c.rows + 2) * c.ldx * (4 if c.dtype == "f32" else 2) <= 40e6
        pos = P.positions(c.rows, "mixed")
        bad = ((pos < 0) | (pos >= P.N_POS)).nonzero().flatten()
        for k in range(2):                                                              # both full passes skip rows and rotate the others ...
            rows = range(k * P.PASS // c.per_row + 1, (k + 1) * P.PASS // c.per_row)
            assert any(int(r) in rows for r in bad) and len([r for r in bad if int(r) in rows]) < len(rows) // 10, (c.name, k)
        assert 0 <= int(pos[-1]) < P.N_POS and int(pos[-1]) != 0 and c.items - 2 * P.PASS < c.per_row          # ... the tail, in the last row, turns
    swiglu = [c for c in P.SWIGLU_CASES if c.multipass]
    assert sorted((c.kind, c.dtype) for c in swiglu) == [("bwd", "bf16"), ("bwd", "f32"), ("fwd", "bf16"), ("fwd", "f32")]
    for c in swiglu:
        assert P.multipass_violations(c.items, c.F // 4) == [], c.name
        assert (c.rows + 2) * max(c.ldu, c.lddu) * 4 <= 40e6
    assert P.multipass_violations(2 * P.PASS, 7) and P.multipass_violations(2 * P.PASS + 256, 7) and P.multipass_violations(2 * P.PASS + 5, 512)


def test_finish_and_swiglu_cases_cover_the_shapes_and_pad_every_stride():
    assert {(c.ks, c.M, c.H, c.hd, c.out) for c in P.FINISH_CASES} == {(ks, M, H, hd, o) for ks in (1, 3, 4) for M in (1, 33, 64)
                                                                      for H, hd in ((3, 8), (2, 24), (2, 64), (1, 128)) for o in ("f32", "bf16")}
    assert all(c.ld_out > 3 * c.E and c.ld_out % 4 == 0 for c in P.FINISH_CASES)
    for hd in (8, 24, 64, 128):
        assert {c.ld_table > c.hd // 2 for c in P.FINISH_CASES if c.hd == hd} == {False, True}
    assert any(c.pos_kind == "above" for c in P.FINISH_CASES) and any(c.pos_kind == "mixed" for c in P.FINISH_CASES)
    small = [c for c in P.SWIGLU_CASES if not c.multipass and not c.edge]
    assert {(c.kind, c.dtype, c.F, c.rows) for c in small} == {(k, d, F, r) for k in ("fwd", "bwd", "splitk") for d in ("f32", "bf16")
                                                              for F in (4, 32, 160, 2052) for r in (1, 5, 65)}
    for c in P.SWIGLU_CASES:
        if c.kind == "bwd":
            assert c.ldu > 2 * c.F and c.lddu > 2 * c.F and c.ldu != c.lddu and c.ldh > c.F
        elif c.kind == "fwd":
            assert c.ldu > 2 * c.F and c.ldh > c.F
        else:
            assert c.ldh > c.F and c.ks in (1, 2, 3, 4)
    assert {c.ks for c in small if c.kind == "splitk"} == {1, 3, 4}
    assert {(c.kind, c.dtype) for c in P.SWIGLU_CASES if c.edge} == {(k, d) for k in ("fwd", "bwd", "splitk") for d in ("f32", "bf16")}


def test_windows_hold_nan_in_input_pads_and_the_sentinel_around_outputs():
    c = P.BY_NAME["swiglu-bwd-bf16-F32-r5"]
    win, _ = P.materialize_swiglu(c)
    for nm in ("u", "dh"):
        bk, vw = win[nm]
        assert P.untouched(bk, vw, fill=P.NAN) and bk.numel() > vw.numel()
    bk, vw = win["out"]
    assert vw.storage_offset() == c.lddu and bk.numel() == (c.rows + 2) * c.lddu and bool((bk == P.SENTINEL).all())
    c = P.BY_NAME["rope-f32-hd8-H3-r5-ldt8-fwd-mixed"]
    win, v = P.materialize_rope(c)
    assert P.untouched(*win["x"]) and P.untouched(*win["cos"], fill=P.NAN) and win["cos"][0].isnan().any()
    assert torch.equal(win["x"][1].double(), v["x"])


# ----------------------------------------------------------------------------------------------------- emulations and their mutants
@pytest.mark.parametrize("family", ["rope", "finish", "swiglu"])
def test_the_plain_emulation_is_accepted_on_every_case(family):
    cases = {"rope": P.ROPE_CASES, "finish": P.FINISH_CASES, "swiglu": P.SWIGLU_CASES}[family]
    assert cases
    for c in cases:
        run(c)


# mutation -> the case that rejects it (and why that one)
KILLERS = {
    "rope": {
        "interleaved_pairs": "rope-f32-hd8-H1-r5-ldt8-inv-mixed",                       # pairs (2i, 2i + 1) instead of (i, i + hd / 2)
        "sin_sign": "rope-f32-hd24-H6-r67-ldt16-fwd-mixed",
        "inverse_ignored": "rope-bf16-hd32-H3-r67-ldt16-inv-mixed",
        "table_stride_half": "rope-bf16-hd16-H6-r67-ldt12-fwd-mixed",                   # ld_table = hd / 2 + 4
        "table_col_plus_half": "rope-f32-hd64-H1-r67-ldt64-fwd-mixed",                  # a table for 2 hd: the columns behind hd / 2 hold numbers
        "table_row_is_r": "rope-bf16-hd128-H6-r67-ldt68-fwd-mixed",
        "clamp_position": "rope-bf16-hd8-H6-r67-ldt8-fwd-mixed",                        # rows 2, 3, 5, 6 are out of range
        "later_passes_skipped": "rope-multipass-bf16-vec8",
        "stride_short_one_block": "rope-multipass-f32-vec4",                            # in place: 256 items a pass rotate twice
        "last_partial_block_dropped": "rope-multipass-bf16-vec4-per_head3",
        "vec4_ignores_per_head": "rope-bf16-hd24-H3-r67-ldt12-inv-mixed",               # per_head = 3
    },
    "finish": {
        "v_rotated": "finish-bf16-H2-hd24-ks3-M33-ldo148-ldt24-mixed",
        "slice_skipped": "finish-f32-H2-hd64-ks3-M33-ldo396-ldt36-mixed",
        "slice_stride_3E": "finish-bf16-H3-hd8-ks3-M33-ldo76-ldt8-mixed",
        "ld_out_ignored": "finish-f32-H1-hd128-ks3-M33-ldo396-ldt68-mixed",
        "table_stride_half": "finish-f32-H2-hd24-ks3-M33-ldo156-ldt16-mixed",
        "table_col_plus_half": "finish-bf16-H2-hd64-ks3-M33-ldo388-ldt64-mixed",
        "table_row_is_r": "finish-f32-H3-hd8-ks3-M33-ldo84-ldt8-mixed",
        "clamp_position": "finish-bf16-H1-hd128-ks3-M33-ldo388-ldt128-mixed",
        "sin_sign": "finish-f32-H2-hd24-ks3-M33-ldo156-ldt16-mixed",
        "interleaved_pairs": "finish-bf16-H2-hd24-ks3-M33-ldo148-ldt24-mixed",
    },
    "swiglu": {
        "gate_up_swapped": "swiglu-fwd-bf16-F160-r5",
        "du_halves_swapped": "swiglu-bwd-bf16-F32-r65",
        "dsilu_is_sigmoid": "swiglu-bwd-bf16-F160-r65",
        "dsilu_is_silu": "swiglu-bwd-f32-F32-r5",
        "pad_column_written": "swiglu-fwd-f32-F2052-r5",
        "later_passes_skipped": "swiglu-multipass-bwd-bf16",
        "last_partial_block_dropped": "swiglu-multipass-fwd-f32",
        "slice_skipped": "swiglu-splitk-bf16-F160-r5-ks3",
        "slice_stride_2F": "swiglu-splitk-f32-F32-r5-ks3",
        "ld_out_ignored": "swiglu-splitk-f32-F4-r65-ks4",
        "lddu_is_ldu": "swiglu-bwd-f32-F160-r5",
        "lddh_is_F": "swiglu-bwd-bf16-F2052-r5",
    },
}


def test_every_mutation_has_a_killer():
    assert set(KILLERS["rope"]) == set(P.ROPE_MUTATIONS) and set(KILLERS["finish"]) == set(P.FINISH_MUTATIONS)
    assert set(KILLERS["swiglu"]) == set(P.SWIGLU_MUTATIONS)


@pytest.mark.parametrize("family,mutation", [(f, m) for f in KILLERS for m in KILLERS[f]])
def test_each_mutant_is_rejected_by_its_named_case(family, mutation):
    c = P.BY_NAME[KILLERS[family][mutation]]
    run(c)                                                   # the case accepts the plain emulation ...
    with pytest.raises(AssertionError) as e:                 # ... and rejects the mutant, saying where
        run(c, mutation)
    assert c.name in str(e.value) and ("row" in str(e.value) or "outside its window" in str(e.value))


def test_the_derivative_mutants_are_rejected_at_small_gates_too():
    """silu' -> sigmoid / silu on the edge table: the zero of silu' and g = +-0 are where a bound relative to the largest element saw nothing."""
    for name in ("swiglu-bwd-f32-edge", "swiglu-bwd-bf16-edge"):
        for mutation in ("dsilu_is_sigmoid", "dsilu_is_silu"):
            with pytest.raises(AssertionError):
                run(P.BY_NAME[name], mutation)
