"""CPU: the references of tests/_seq_probe.py reproduce the committed fixtures and the oracle, the case tables cover what they claim,
and the acceptance functions the GPU probes use (`check_rows`, `check_labels`, `check_embed`, `check_move`, `check_transpose`,
`check_gated`, `check_vit`) accept a plain emulation of every kernel and reject each of its one-line mutations.
"""
import numpy as np
import pytest
import torch

import oracle
import _incontext_ref as IR
import _seq_probe as S
from conftest import load_golden


# ------------------------------------------------------------------------------------------------------------------- helpers
def test_int64_windows_can_be_guarded():
    bk, vw = S.window(2, 3, 3, torch.int64, elem_offset=2, fill=S.POISON_I64)
    assert S.untouched(bk, vw, S.POISON_I64)
    vw.fill_(-100)
    assert S.untouched(bk, vw, S.POISON_I64)
    for idx in (0, 1, 2 + 6, bk.numel() - 1):
        b = bk.clone()
        b[idx] = -100
        assert not S.untouched(b, b.as_strided((2, 3), (3, 1), 2), S.POISON_I64), idx
    b = bk.clone()
    b[0] = S.POISON_I64 + (1 << 40)                         # all 64 bits are compared
    assert not S.untouched(b, b.as_strided((2, 3), (3, 1), 2), S.POISON_I64)


def test_poisons_are_outside_every_range_a_case_uses():
    assert S.POISON_ID > S.VOCAB and S._i32(S.POISON_ID) > S.VOCAB and S.POISON_ID != 0
    assert S.POISON_I32 < -(1 << 20) and S.POISON_I64 < -(1 << 40)           # no prefix row, label, mask bit, position or count
    assert S.TEXT_HI < S.SPECIAL - max(S.FEWSHOT_NIMG) and S.SPECIAL + 1 < S.VOCAB


# ------------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("case", ["z", "f", "s"])
def test_references_reproduce_insert_prefix_fixture(case):
    """Mask through ref_fewshot_rows, embeddings through ref_embed: every text token is renamed to the number of its own (row, column),
    which makes the fixture's per-position text embeddings a table."""
    z = load_golden("insert_prefix.npz")
    tok, text, pp, mask = (z[f"{case}_{k}"] for k in ("tok", "text", "pp", "mask"))
    B, T = tok.shape
    _, n_img, L, E = pp.shape
    special = 32099
    sent = IR.is_sentinel(tok, n_img, special)
    assert B * T < special - n_img
    renamed = np.where(sent, tok, np.arange(B * T).reshape(B, T))
    src, m, pos, status = S.ref_fewshot_rows(renamed, mask, L, n_img, special, 0)
    assert (status == n_img).all()
    assert np.array_equal(m, z[f"{case}_out_mask"])
    assert np.array_equal(pos, np.tile(np.arange(m.shape[1]), (B, 1)))
    emb = S.ref_embed(src.reshape(-1), None, torch.from_numpy(text).reshape(B * T, E), torch.from_numpy(pp).reshape(-1, E), None)
    assert torch.equal(emb.reshape(B, -1, E), torch.from_numpy(z[f"{case}_emb"]).double())


def test_ref_labels_reproduces_label_mask_fixture():
    z = load_golden("label_mask.npz")
    got = S.ref_labels(z["input_ids"], 0, int(z["pad_id"]), int(z["bos_id"]), 0)
    assert np.array_equal(got, z["labels"])
    got = S.ref_labels(z["input_ids"], 2, int(z["pad_id"]), int(z["bos_id"]), 1)
    assert (got[:, :2] == -100).all() and np.array_equal(got[:, 2:], np.where(z["input_ids"] == z["pad_id"], -100, z["input_ids"]))


def test_ref_fewshot_rows_is_the_oracles_walk_on_every_well_formed_row():
    seen = 0
    for c in S.FEWSHOT_CASES:
        tokens, qmask, _ = S.row_inputs(c)
        src, mask, pos, status = S.ref_fewshot_rows(tokens, qmask, c.L, c.n_img, S.SPECIAL, c.pos_mode)
        rows = S.well_formed(c, tokens)
        assert [b for b in range(c.B) if status[b] == c.n_img] == rows
        if not rows:
            continue
        seen += len(rows)
        code = torch.tensor([[[[-(1 + (b * c.n_img + n) * c.L + l)] for l in range(c.L)] for n in range(c.n_img)] for b in rows], dtype=torch.float64)
        emb, msk = oracle.insert_prefix_into_input(c.L, c.n_img - 1, torch.from_numpy(tokens[rows]), torch.from_numpy(tokens[rows])[..., None].double(),
                                                   code, torch.from_numpy(qmask[rows]), special_token_id=S.SPECIAL)
        assert np.array_equal(emb[..., 0].long().numpy(), src[rows]), c.name
        assert np.array_equal(msk.numpy(), mask[rows]), c.name
        want = torch.cumsum(msk, 1) * msk - 1 + 2 if c.pos_mode else torch.arange(msk.shape[1]).expand_as(msk)
        assert np.array_equal(want.numpy(), pos[rows]), c.name
    assert seen >= 4 * len(S.FEWSHOT_CASES)


def test_ref_fewshot_rows_lays_text_out_as_expand_labels_does():
    """tests/_incontext_ref.expand_labels (the label layout of training on interleaved rows) with the token ids as labels: the text of
    every row, the over-full and under-full ones included, sits where ref_fewshot_rows puts it."""
    for c in S.FEWSHOT_CASES:
        tokens, qmask, _ = S.row_inputs(c)
        src = S.ref_fewshot_rows(tokens, qmask, c.L, c.n_img, S.SPECIAL, 0)[0]
        out, scored = IR.expand_labels(tokens, tokens, c.L, c.n_img, S.SPECIAL)
        assert np.array_equal(out, np.where(src > 0, src, -100)), c.name
        assert np.array_equal(scored, (src > 0).sum(1)), c.name


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_fewshot_table_covers_its_layouts():
    cs = S.FEWSHOT_CASES
    assert {c.T for c in cs} == {1, 63, 64, 65, 130} and {c.L for c in cs} == {1, 2, 10} and {c.n_img for c in cs} == {1, 3, 5}
    assert {c.pos_mode for c in cs} == {0, 1} and all(c.B == 8 for c in cs)
    facts = {c.name: set().union(*S.row_inputs(c)[2]) for c in cs}
    every = set().union(*facts.values())
    want = {n for n, *_ in S.FEWSHOT_ROWS} | {"mask:right", "mask:left", "mask:holes", "sent@0", "sent@63", "sent@64", "sent@T-1", "sent@63|64",
                                              "near-ids-as-text", "mask-0-on-sentinel", "under-full", "over-full", "twice-n_img",
                                              "every-id-of-the-window"}
    assert want <= every, want - every
    for edge in ("sent@63", "sent@64", "sent@63|64", "sent@T-1", "sent@0", "mask:left", "mask:holes", "twice-n_img", "under-full"):
        for L in S.FEWSHOT_L:            # every chunk-edge layout under OPT positions, with and without a shift of the text behind it
            assert any(edge in facts[c.name] for c in cs if c.pos_mode == 1 and c.L == L and c.T > 64), (edge, L)
    assert any("every-id-of-the-window" in facts[c.name] for c in cs if c.n_img == 5)
    for c in cs:                         # the expanded row crosses a chunk wherever the input row does
        assert c.S == c.T + (c.L - 1) * c.n_img
    assert any(c.S > 128 for c in cs if c.pos_mode == 1)


def test_prefix_table_covers_its_layouts():
    cs = S.PREFIX_CASES
    assert {(c.L, c.T) for c in cs} == {(0, 5), (10, 0), (1, 63), (10, 54), (10, 55), (70, 70)}
    for L, T in S.PREFIX_LT:
        got = {(c.stride, c.offset, c.pos_mode) for c in cs if (c.L, c.T) == (L, T)}
        assert got == {(s, o, pm) for s, o in ((L, 0), (3 * L, L), (3 * L, 2 * L)) for pm in (0, 1)}
    for c in cs:
        assert c.stride >= c.L and c.offset + c.L <= max(c.stride, c.L)
        assert {"mask:right", "mask:left", "mask:holes"} <= set().union(*S.row_inputs(c)[2])
    assert {c.S for c in cs} >= {5, 64, 65, 140}             # part of a chunk, exactly one, one more, three


def test_labels_table_covers_its_layouts():
    cs = S.LABELS_CASES
    assert {c.T for c in cs} == {1, 64, 65, 150} and {c.L for c in cs} == {0, 3, 70} and {c.mode for c in cs} == {0, 1}
    assert any(c.bos == -1 and c.mode == 0 for c in cs)
    names = {T: S.label_ids(S.LabelsCase("x", T, 0, 0))[1] for T in S.LABELS_T}
    assert set(S.LABEL_ROWS) == set(names[150]) == set(names[65])
    assert {"pad@0", "pad@T-1", "no-pad", "all-pad"} <= set(names[1]) and "pad@63" in names[64] and "bos@63" in names[64]
    ids, nm = S.label_ids(S.LabelsCase("x", 150, 0, 0))
    for name, row in zip(nm, ids):
        pads, bos = np.flatnonzero(row == S.PAD), np.flatnonzero(row == S.BOS)
        if name.startswith("pad@"):
            assert pads[0] == (149 if name == "pad@T-1" else int(name[4:]))
        if name.startswith("bos@"):
            assert bos[0] == int(name[4:]) and pads[0] > bos[0] + 1
        if name == "two-bos-before-the-pad":
            assert (bos < pads[0]).sum() == 2
        if name == "bos-only-after-the-pad":
            assert bos.size and bos[0] > pads[0]
        if name == "no-pad":
            assert pads.size == 0 and bos.size
        if name == "all-pad":
            assert pads.size == 150


def test_embed_table_covers_its_layouts():
    cs = S.EMBED_CASES
    assert {c.E for c in cs} == {4, 1020, 1024, 1028, 2560} and {c.dtype for c in cs} == {"f32", "bf16"} and {c.wpe for c in cs} == {True, False}
    R = S.embed_rows()
    src, pos = R["src"], R["pos"]
    assert src.min() >= -R["n_prefix"] and src.max() < S.VOCAB and pos.min() >= 0 and pos.max() < R["n_pos"]      # every id inside its table
    assert (np.diff(pos) < 0).any() and (pos == 1).sum() > 8                       # OPT's offset, repeated 1s at masked positions
    assert (np.diff(np.sign(src)) != 0).sum() > 16                                 # prefix and token rows interleave
    named = {-int(s) - 1 for s in src if s < 0}
    assert 0 < len(named) < R["n_prefix"] and len(named) == int((src < 0).sum())   # some prefix rows unnamed, none named twice
    for c in cs:
        lds = [c.ld(o) for o in ("wte", "prefix", "wpe", "x", "dx", "dprefix")]
        assert len(set(lds)) == 6 and all(ld > c.E and ld % 4 == 0 for ld in lds)
        bufs, v = S.materialize_embed(c)
        for nm in ("wte", "prefix", "dx") + (("wpe",) if c.wpe else ()):
            assert 0 < v[nm].abs().max().item() <= S.LIM[c.dtype] and torch.equal(bufs.win[nm][1].double(), v[nm])
    assert any(c.E > 2048 for c in cs)                                             # a third 1024-column pass


def test_move_table_covers_its_layouts():
    cs = S.MOVE_CASES
    assert {c.cols for c in cs if c.dtype == "bf16"} == {8, 2040, 2048, 2056} and {c.cols for c in cs if c.dtype == "f32"} == {4, 1020, 1024, 1028}
    assert {c.n for c in cs} == {1, 7, 300} and {c.scatter for c in cs} == {True, False}
    for c in cs:
        assert c.ld_src != c.ld_dst and min(c.ld_src, c.ld_dst) > c.cols
        assert S.move_accepts(c.dtype, c.cols, c.ld_src, c.ld_dst, 0, 0)
        idx = S.move_index(c)
        assert idx.min() >= 0 and idx.max() < c.other_rows and len(idx) == c.n
        assert len(set(idx.tolist())) == (c.n if c.scatter or c.n == 1 else c.n - 1)          # scatter: no index twice; gather: one repeated
    for r in S.MOVE_REJECTED:
        assert not S.move_accepts(*r), r


def test_transpose_table_states_the_kernel_of_every_case():
    cs = S.TRANSPOSE_CASES
    assert {(c.rows, c.cols) for c in cs} == {(1, 1), (63, 65), (64, 64), (65, 63), (60, 68), (132, 68), (4, 260)}
    assert {c.src_off for c in cs} == {0, 4, 2, 1} == {c.dst_off for c in cs}
    for c in cs:
        assert c.ld_src > c.cols and c.ld_dst > c.rows
        aligned = c.src_off in (0, 4) and c.dst_off in (0, 4)
        fours = (c.rows, c.cols) in ((64, 64), (60, 68), (132, 68), (4, 260))
        assert c.fast == (c.dtype == "bf16" and aligned and fours), c.name
    fast = {(c.rows, c.cols) for c in cs if c.fast}
    slow = {(c.rows, c.cols) for c in cs if c.dtype == "bf16" and not c.fast}
    ragged_both = lambda shapes: any(r % 64 and cl % 64 and (r > 64 or cl > 64) for r, cl in shapes)
    assert ragged_both(fast) and ragged_both(slow)
    assert {(c.src_off, c.dst_off) for c in cs if c.fast} == {(0, 0), (4, 0), (0, 4)}
    assert {(c.src_off, c.dst_off) for c in cs if c.dtype == "bf16" and (c.rows, c.cols) == (132, 68) and not c.fast} == {(2, 0), (1, 0), (0, 2), (0, 1)}


def test_gated_table_covers_its_layouts():
    cs = S.GATED_CASES
    shapes = {(c.rows, c.F, c.ldu, c.ldh, c.lddh, c.lddu) for c in cs}
    assert shapes == {(1, 4, 8, 4, 4, 8), (37, 136, 280, 140, 144, 276), (520, 4100, 8204, 4104, 4100, 8200)}
    assert {(c.dtype, c.act) for c in cs if c.exact} == {(d, a) for d in ("f32", "bf16") for a in ("none", "relu")}
    assert {(c.dtype, c.act, c.rows) for c in cs if not c.exact} == {(d, a, r) for d in ("f32", "bf16") for a in ("tanh", "gelu_new", "quick_gelu") for r in (37, 520)}
    per_pass = S.GATED_BLOCKS * S.GATED_THREADS
    assert 520 * 4100 // 4 == 533000 > per_pass and per_pass % (4100 // 4) != 0            # a second pass that starts inside a row
    assert any(c.ldu > 2 * c.F and c.ldu // 2 != c.F for c in cs) and all(c.ldu >= 2 * c.F and c.lddu >= 2 * c.F for c in cs)
    for c in cs:
        if c.rows > 37 and c.dtype == "f32":
            continue                                          # (the same generator and ranges as the bf16 case of this shape)
        _, v = S.materialize_gated(c)
        ref = S.reference_gated(c, v)
        if c.exact:
            for x in (ref["h"], ref["du"]):
                assert torch.equal(x, x.round()) and x.abs().max().item() <= 64
        else:
            assert v["u"].abs().max().item() <= 3 and v["dh"].abs().max().item() <= 3
            assert torch.equal(v["u"], v["u"].to(S.DT[c.dtype]).double())


def test_vit_table_covers_its_layouts():
    cs = S.VIT_CASES
    assert {(c.img, c.ps, c.ldp) for c in cs if c.kind == "patchify"} == {(28, 14, 588), (28, 14, 608), (32, 16, 768)}
    assert {(c.W, c.n_patch) for c in cs if c.kind == "assemble"} == {(W, n) for W in (4, 1028, 1280) for n in (1, 5)}
    assert all(c.B == 2 for c in cs) and {c.dtype for c in cs} == {"f32", "bf16"}
    assert all(c.ldpe > c.W and c.ldx > c.W and c.ldpe != c.ldx for c in cs if c.kind == "assemble")


# ------------------------------------------------------------------------------------------------------ emulations and mutations
def run(group, c, mutation=None):
    _, mat, ref, emu, chk = S.GROUPS[group]
    bufs, v = mat(c)
    want = ref(c, v)
    emu(c, bufs, mutation)
    chk(c, want, bufs)


@pytest.mark.parametrize("group", list(S.GROUPS))
def test_plain_emulation_passes_every_check(group):
    for c in S.GROUPS[group][0]:
        run(group, c)
    if group == "gated":
        assert len(S.WORST) == 12 and max(S.WORST.values()) <= 1.0


@pytest.mark.parametrize("group", list(S.GROUPS))
def test_an_untouched_output_fails_every_check(group):
    """The checks compare: outputs left at their fill are no result."""
    _, mat, ref, _, chk = S.GROUPS[group]
    c = S.GROUPS[group][0][-1]
    bufs, v = mat(c)
    with pytest.raises(AssertionError):
        chk(c, ref(c, v), bufs)


def test_mutation_list_is_the_issues():
    assert len(S.MUTATIONS) == 23 and set(S.MUTATIONS) == set(S.ROW_MUTATIONS + S.LABEL_MUTATIONS + S.EMBED_MUTATIONS + S.MOVE_MUTATIONS
                                                               + S.TRANSPOSE_MUTATIONS + S.GATED_MUTATIONS + S.VIT_MUTATIONS)


@pytest.mark.parametrize("mutation", sorted(S.MUTATIONS))
def test_every_mutation_is_rejected(mutation):
    for group in S.MUTATIONS[mutation]:
        rejected = []
        for c in S.GROUPS[group][0]:
            try:
                run(group, c, mutation)
            except AssertionError as e:
                rejected.append(f"{c.name}: {e}")
                break
        assert rejected, f"{mutation}: no {group} case notices it"
