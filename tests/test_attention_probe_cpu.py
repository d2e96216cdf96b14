"""The attention probes checked on their own (no GPU): every property tests/_attention_probe.py states of its builders, the bf16
emulation that must pass the acceptance check, and the mutation check - a reference that is wrong by one key (or one bias column)
must be rejected, forward and backward, which is the evidence that the GPU tests would fail on a kernel that is subtly wrong.
The same for the shared-prompt decode step (a model that reads the call's buffers with one index wrong), the two-segment merge (one
log-sum-exp index wrong) and the scoring flow (three roundings inside the bound)."""
import math
import pathlib
import re

import pytest
import torch

import _attention_probe as ap

FORWARD_ONLY = set(ap.RESIDENT_CASES + ap.DECODE_CASES + ap.DECODE_REL_CASES)
IDS = [c.id for c in ap.ALL_CASES]


def setup(case):
    km = ap.key_mask(case)
    keep = ap.visible(case, km)
    return km, keep, ap.rows_checked(case, keep), ap.bias_matrix(case)


def is_bf16(x, slack=0.0):
    """Exactly representable in bf16; ``slack``: up to the losing keys' weights (below 1e-27 each, Probe B)."""
    return off_bf16(x) <= slack


def off_bf16(x):
    return (x.to(torch.bfloat16).double() - x).abs().max().item()


@pytest.mark.parametrize("case", ap.ALL_CASES, ids=IDS)
def test_rows_without_a_visible_key_are_the_stated_ones(case):
    km, keep, ok, _ = setup(case)
    empty = int((~keep.any(-1)).sum())
    assert empty == case.empty_rows
    assert empty == 0 or case.mask == "left"
    exist = torch.ones(case.B, case.Sq, dtype=torch.bool) if case.lens is None else torch.arange(case.Sq)[None] < torch.tensor(case.lens)[:, None]
    assert torch.equal(ok, keep.any(-1)[:, 0] & exist)                     # nothing else is left out
    if km is not None:
        assert km.dtype == torch.int32 and km.shape == (case.B, case.Sk) and bool(km.any(-1).all())
    if case.mask == "holes":
        assert bool((km[:, -1] == 1).all()) and (case.Sk < 17 or 0.5 < km.float().mean().item() < 0.9)
    if case.mask == "left" and case.Sk >= 129:
        assert int(km[1, :70].sum()) == 0 and int(km[1, 64:128].sum()) == 58  # sample 1: tile 0 fully masked, tile 1 partly


def test_the_masks_are_the_stated_ones():
    km = ap.key_mask(ap.Case(3, 1, 20, 20, 64, False, "right"))
    assert km.sum(-1).tolist() == [20, 16, 13]
    km = ap.key_mask(ap.Case(2, 1, 129, 129, 64, False, "left"))
    assert km[0].tolist() == [0] * 5 + [1] * 124 and km[1].tolist() == [0] * 70 + [1] * 59
    assert ap.key_mask(ap.Case(2, 1, 64, 64, 64, False, "left"))[1].tolist() == [0] * 9 + [1] * 55


@pytest.mark.parametrize("case", [c for c in ap.ALL_CASES if c.buckets], ids=[c.id for c in ap.ALL_CASES if c.buckets])
def test_bias_table(case):
    rel, zero = ap.rel_table(case)
    assert rel.shape == (case.H, 2 * case.Sk - 1 + 2 * ap.REL_MARGIN) and rel.dtype == torch.float32
    assert torch.equal(rel * 8, (rel * 8).round()) and rel.abs().max() <= 4
    vals = ap.bucket_values(case.H)
    for h in range(case.H):
        assert len(set(vals[h].tolist())) == 32                           # different per bucket within a head
        near = rel[h, zero - 7:zero + (8 if case.buckets == "bi" else 1)]
        assert len(set(near.tolist())) == near.numel()                      # ... so different per offset next to the diagonal
        assert all(not torch.equal(rel[h], rel[g]) for g in range(h))
    if case.buckets == "one":
        assert bool((rel[:, zero:] == rel[:, zero:zero + 1]).all())         # keys ahead of the query share bucket 0
    # the matrix is rel[h, key - query position + zero], the query sitting at i + Sk - Sq
    b = ap.bias_matrix(case)
    i, j = case.Sq - 1, 0
    assert b[0, 1, i, j].item() == rel[1, j - (case.Sk - 1) + zero].item()


@pytest.mark.parametrize("case", ap.ALL_CASES, ids=IDS)
def test_probe_a_reads_p_out_element_by_element(case):
    km, keep, ok, bias = setup(case)
    B, H, Sq, Sk, hd = case.B, case.H, case.Sq, case.Sk, case.hd
    heads = (1.0 + torch.arange(H, dtype=torch.float64))[None, None, :, None]
    p = None
    cols = []
    for pr in ap.probe_a_forward(case):
        assert all(is_bf16(t) for t in (pr.q, pr.k, pr.v)) and torch.isfinite(pr.k).all() and pr.k.abs().max() > 1
        ref = ap.reference(pr.q, pr.k, pr.v, None, keep, bias, pr.scale)
        p = ref.p
        cols.append(ref.val["o"] / heads)
        assert torch.equal(ref.mag["o"], ref.val["o"])
    got = torch.cat(cols, -1)[..., :Sk].permute(0, 2, 1, 3)                                     # [B, H, Sq, Sk]
    assert torch.allclose(got, p, rtol=0, atol=1e-15)
    okr = ok[:, None, :, None]
    if bias is None:
        count = keep.sum(-1, keepdim=True).clamp(min=1).double()
        assert torch.allclose(p, (keep / count).expand_as(p) * okr.double() + p * (~okr), rtol=0, atol=1e-15)
        assert torch.allclose(ref.lse * ok[:, None], (torch.log(count)[..., 0] * ok[:, None]).expand_as(ref.lse), rtol=0, atol=1e-12)
    else:
        s = torch.where(keep, bias.expand(B, H, Sq, Sk), torch.full((1,), -math.inf, dtype=torch.float64))
        assert torch.allclose(p, torch.softmax(s, -1), rtol=0, atol=1e-15)
    assert bool((p[~keep.expand_as(p)] == 0).all())
    if case in FORWARD_ONLY:
        return
    dv_cols, dq_cols, a = [], [], None
    for pr in ap.probe_a_backward(case, ok):
        assert all(is_bf16(t) for t in (pr.q, pr.k, pr.v, pr.do))
        ref = ap.reference(pr.q, pr.k, pr.v, pr.do, keep, bias, pr.scale)
        assert not ref.val["dk"].any()
        if pr.name.startswith("A.dkv"):
            dv_cols.append(ref.val["dv"])                                                       # [B, Sk, H, hd]: P[b, h, c hd + d, j]
            assert not ref.val["dq"].any()
        else:
            dq_cols.append(ref.val["dq"] / pr.scale)
            a = pr.v[..., 0].permute(0, 2, 1)[:, :, None, :]                                    # [B, H, 1, Sk]
    pt = torch.cat(dv_cols, -1)[..., :Sq].permute(0, 2, 3, 1)
    assert torch.allclose(pt, p * okr, rtol=0, atol=1e-15)
    want = p * (a - (p * a).sum(-1, keepdim=True)) * okr
    assert torch.allclose(torch.cat(dq_cols, -1)[..., :Sk].permute(0, 2, 1, 3), want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("case", ap.ALL_CASES, ids=IDS)
def test_probe_b_is_sharp_and_exact_in_bf16(case):
    km, keep, ok, bias = setup(case)
    if case.Sq == 1:                                                                            # decode steps: one-hot on the stated keys
        for pr in [pr for pr in ap.probes(case, keep, ok, False) if pr.name.startswith("B.")]:
            assert all(is_bf16(t) for t in (pr.q, pr.k, pr.v)) and pr.scale == 1.0 and pr.do is None
            ref = ap.reference(pr.q, pr.k, pr.v, None, keep, None, pr.scale)
            for b in range(case.B):
                vis = torch.nonzero(keep[b, 0, 0])[:, 0].tolist()
                t = ap.DECODE_PICKS[pr.name[2:]](b, 0, vis)
                assert t in vis and t == {"last": case.Sk - 1, "first": vis[0], "edge": max([j for j in vis if j <= 64] + vis[:1])}[pr.name[2:]]
                row = ref.p[b, :, 0].clone()
                assert bool((row[:, t] == 1.0).all())
                row[:, t] = 0
                assert row.max().item() < 1e-27
            assert off_bf16(ref.p) <= 1e-27 and off_bf16(ref.val["o"]) <= 1e-24
        assert (len([pr for pr in ap.probes(case, keep, ok, False) if pr.name.startswith("B.")]) == 3) == (case.buckets is None)
        return
    pr = ap.probe_b(case, keep, ok, backward=case not in FORWARD_ONLY)
    assert all(is_bf16(t) for t in (pr.q, pr.k, pr.v)) and pr.scale == 1.0
    assert not pr.k[..., ap.CODE_BITS:].any() and not pr.q[..., ap.CODE_BITS:].any()
    ref = ap.reference(pr.q, pr.k, pr.v, pr.do, keep, None, pr.scale)                           # the plain scores, also for the rel cases
    p = ref.p
    two = 0
    for b in range(case.B):
        for i in range(case.Sq):
            if not ok[b, i]:
                assert not pr.q[b, i].any() and (pr.do is None or not pr.do[b, i].any())
                continue
            t1, t2 = ap.select_targets(keep[b, 0, i], i)
            assert bool(keep[b, 0, i, t1]) and (t2 is None or (bool(keep[b, 0, i, t2]) and (t1 + 1) ^ (t2 + 1) == 1))
            if t2 is None:
                partner = ((t1 + 1) ^ 1) - 1
                assert not (0 <= partner < case.Sk and bool(keep[b, 0, i, partner]))               # two-hot whenever it can be
            row = p[b, :, i].clone()
            for t in (t1, t2):
                if t is not None:
                    assert bool((row[:, t] == (1.0 if t2 is None else 0.5)).all())
                    row[:, t] = 0
            assert row.max().item() < 1e-27
            two += t2 is not None
    assert two > 0 or case.Sk == 1 or case.Sq == 1
    live = ok[:, None, :, None].double()                                                        # (rows packing leaves out hold q = 0)
    assert off_bf16(p * live) <= 1e-27 and off_bf16(ref.val["o"] * ok[:, :, None, None]) <= 1e-24
    if pr.do is not None:
        assert is_bf16(pr.do)
        if case.hd <= 128:
            assert is_bf16(ref.val["ds"], 1e-24)
    if case.causal and case.Sq == case.Sk >= 65 and case.mask != "holes":                       # row 64 asks for its last key: the pair (63, 64)
        b = 0
        assert bool(ok[b, 64]) and set(ap.select_targets(keep[b, 0, 64], 64)) == {63, 64}
        assert bool(((p[b, :, 64, 63] == 0.5) & (p[b, :, 64, 64] == 0.5)).all())


def test_reference_matches_autograd():
    case = ap.Case(2, 2, 9, 13, 16, True, "holes", "one")
    km, keep, ok, bias = setup(case)
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(2, n, 2, 16, generator=g, dtype=torch.float64) for n in (9, 13, 13, 9))
    ref = ap.reference(q, k, v, do, keep, bias, 0.3)
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bihd,bjhd->bhij", qq, kk) * 0.3 + bias
    s = torch.where(keep, s, torch.full_like(s, torch.finfo(torch.float32).min))
    o = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, -1), vv)
    o.backward(do)
    for name, want in (("o", o.detach()), ("dq", qq.grad), ("dk", kk.grad), ("dv", vv.grad)):
        assert torch.allclose(ref.val[name], want, rtol=0, atol=1e-12), name
        assert bool((ref.mag[name] >= ref.val[name].abs() - 1e-12).all()), name
    assert torch.allclose(ref.lse, torch.logsumexp(s, -1).detach(), rtol=0, atol=1e-12)
    again = ap.reference(q, k, v, do, keep, bias, 0.3, fwd=ref)                                 # rebuilt from lse, as a backward kernel does
    for name in ("dq", "dk", "dv"):
        assert torch.allclose(again.val[name], ref.val[name], rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", ap.ALL_CASES, ids=IDS)
def test_bf16_emulation_passes_the_acceptance_check(case):
    """A kernel model that rounds P, dS and every output to bf16 (delta taken from the rounded output) stays within the bound."""
    km, keep, ok, bias = setup(case)
    worst = 0.0
    for pr in ap.probes(case, keep, ok, backward=case not in FORWARD_ONLY):
        ref = ap.reference(pr.q, pr.k, pr.v, pr.do, keep, bias, pr.scale)
        emu = ap.reference(pr.q, pr.k, pr.v, pr.do, keep, bias, pr.scale, rnd=ap._bf16)
        got = {n: emu.val[n] for n in pr.outputs}
        got["lse"] = emu.lse.float().double()
        worst = max(worst, ap.check(got, ref, torch.bfloat16, ok, pr.exact_zero, what=pr.name))
    print(f"{case.id}: worst error / bound of the bf16 emulation {worst:.3f}")
    assert 0 < worst <= 1.0 or case.Sk == 1


# The mutations that change nothing in a case (no causal diagonal to move, no bias to shift, key Sk - 1 visible already, ...): every
# other (case, mutation) pair must be rejected, and a pair listed here must indeed change nothing.
NO_EFFECT_BY_CASE = {
    '2x2x17x17x64-causal-right': ('bias+1', 'bias-1'),
    '2x2x64x64x64-causal-left': ('last_key_visible', 'tile_first_key_dropped', 'bias+1', 'bias-1'),
    '2x2x65x65x64-full-holes': ('diag+1', 'diag-1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x1x129x129x128-causal-left': ('last_key_visible', 'bias+1', 'bias-1'),
    '2x2x170x170x64-full-right': ('diag+1', 'diag-1', 'bias+1', 'bias-1'),
    '1x2x70x200x80-causal-holes': ('last_key_visible', 'bias+1', 'bias-1'),
    '2x2x100x100x96-full-left': ('diag+1', 'diag-1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x1x40x40x200-full-holes': ('diag+1', 'diag-1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x2x20x37x16-causal-holes': ('last_key_visible', 'bias+1', 'bias-1'),
    '1x2x65x65x64-full-none': ('diag+1', 'diag-1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '1x2x97x97x64-full-none': ('diag+1', 'diag-1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '1x2x257x257x64-full-none': ('diag+1', 'diag-1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x2x170x170x64-full-right-bi': ('diag+1', 'diag-1'),
    '1x2x129x129x64-causal-none-one': ('last_key_visible', 'tile_mask_late'),
    '2x2x100x100x128-full-left-bi': ('diag+1', 'diag-1', 'last_key_visible'),
    '2x2x5x150x64-causal-none-one': ('last_key_visible', 'tile_mask_late'),
    '2x3x9x9x80-full-holes-bi': ('diag+1', 'diag-1', 'last_key_visible', 'tile_first_key_dropped'),
    '2x3x1x1x64-causal-left': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x3x1x1x64-causal-holes': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x3x1x1x80-causal-left': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x3x1x1x80-causal-holes': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x3x1x1x128-causal-left': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x3x1x1x128-causal-holes': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x3x1x64x64-causal-left': ('diag+1', 'last_key_visible', 'tile_first_key_dropped', 'bias+1', 'bias-1'),
    '2x3x1x64x64-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x64x80-causal-left': ('diag+1', 'last_key_visible', 'tile_first_key_dropped', 'bias+1', 'bias-1'),
    '2x3x1x64x80-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x64x128-causal-left': ('diag+1', 'last_key_visible', 'tile_first_key_dropped', 'bias+1', 'bias-1'),
    '2x3x1x64x128-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x65x64-causal-left': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x65x64-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x65x80-causal-left': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x65x80-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x65x128-causal-left': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x65x128-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x200x64-causal-left': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x200x64-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x200x80-causal-left': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x200x80-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x200x128-causal-left': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x3x1x200x128-causal-holes': ('diag+1', 'last_key_visible', 'bias+1', 'bias-1'),
    '2x2x1x1x64-causal-none-one': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x2x1x1x64-causal-holes-one': ('diag+1', 'last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '2x2x1x65x64-causal-none-one': ('diag+1', 'last_key_visible', 'tile_mask_late'),
    '2x2x1x65x64-causal-holes-one': ('diag+1', 'last_key_visible'),
    '2x2x1x170x64-causal-none-one': ('diag+1', 'last_key_visible', 'tile_mask_late'),
    '2x2x1x170x64-causal-holes-one': ('diag+1', 'last_key_visible'),
    '4x2x70x70x64-causal-packed-70_1_64_17': ('last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
    '4x2x64x64x64-causal-packed-64_49_16_1': ('last_key_visible', 'tile_mask_late', 'bias+1', 'bias-1'),
}
NO_EFFECT = {(c, m) for c, ms in NO_EFFECT_BY_CASE.items() for m in ms}


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", ap.ALL_CASES, ids=IDS)
def test_a_reference_wrong_by_one_key_is_rejected(case):
    km, keep, ok, bias = setup(case)
    backward = case not in FORWARD_ONLY
    truth = [(pr, ap.reference(pr.q, pr.k, pr.v, pr.do, keep, bias, pr.scale)) for pr in ap.probes(case, keep, ok, backward)]
    z = lambda n: torch.zeros(case.B, n, case.H, 1, dtype=torch.float64)
    p_true = ap.reference(z(case.Sq), z(case.Sk), z(case.Sk), None, keep, bias, 1.0).p * ok[:, None, :, None]
    for mut in ap.MUTATIONS:
        keep_m, bias_m = ap.mutate(case, km, mut)
        p_mut = ap.reference(z(case.Sq), z(case.Sk), z(case.Sk), None, keep_m, bias_m, 1.0).p * ok[:, None, :, None]
        altered = (p_mut - p_true).abs().max().item() > 1e-12
        assert altered != ((case.id, mut) in NO_EFFECT), f"{mut}: altered = {altered}"
        if not altered:
            continue

        def forward_wrong(pr, ref):
            bad = ap.reference(pr.q, pr.k, pr.v, None, keep_m, bias_m, pr.scale)
            ap.check({"o": bad.val["o"], "lse": bad.lse}, ref, torch.bfloat16, ok, pr.exact_zero)

        def backward_wrong(pr, ref):        # a right forward (its lse and output), then a backward with the wrong visible set / bias
            bad = ap.reference(pr.q, pr.k, pr.v, pr.do, keep_m, bias_m, pr.scale, fwd=ref)
            ap.check({n: bad.val[n] for n in ("dq", "dk", "dv")}, ref, torch.bfloat16, ok, pr.exact_zero)

        assert any(_rejected(lambda: forward_wrong(pr, ref)) for pr, ref in truth), f"{mut}: the forward probes accept it"
        if backward:
            assert any(_rejected(lambda: backward_wrong(pr, ref)) for pr, ref in truth if pr.do is not None), f"{mut}: the backward probes accept it"


# ------------------------------------------------------------------------------------------------------------------- shared prompt
SHARED_IDS = [c.id for c in ap.SHARED_CASES]
SHARED_SRC = pathlib.Path(__file__).resolve().parents[1] / "explicit-alignment-for-vqa-tasks_amd" / "csrc" / "attention_decode_shared.hip"


def _f32(x):
    return x.float().double()


def test_shared_table_follows_the_kernel_source():
    """SH_WPH, SH_U and the lanes per key of each launch line, read from the source: a retuned kernel fails here, not silently."""
    src = SHARED_SRC.read_text()
    consts = re.search(r"constexpr int SH_WPH = (\d+), SH_U = (\d+), SH_GMAX = (\d+);", src)
    assert consts and (int(consts[1]), int(consts[2])) == (ap.SH_WPH, ap.SH_U) and int(consts[3]) == 8
    assert "KPI = 64 / LPK" in src and "STEP = KPI * SH_WPH * SH_U" in src and "c = SH_U / G" in src and "i0 += c * SH_WPH * KPI" in src
    launches = re.findall(r"(if \(hd <= (\d+)\)|else) hipLaunchKernelGGL\(\(attn_decode_shared_kernel<(\w+), (\d+)>\)", src)
    assert [(ty, int(lpk)) for _, _, ty, lpk in launches] == [("bf16_t", 8), ("bf16_t", 16), ("float", 16), ("float", 32)]
    assert [edge for _, edge, _, _ in launches] == ["64", "", "64", ""]
    for (dtype, narrow), lpk in zip((("bf16", 64), ("bf16", 65), ("fp32", 64), ("fp32", 65)), (8, 16, 16, 32)):
        assert ap.shared_lpk(dtype, narrow) == lpk
    for sc in ap.SHARED_CASES:
        lpk = ap.shared_lpk(sc.dtype, sc.hd)
        assert sc.kpi == 64 // lpk and sc.step == sc.kpi * ap.SH_WPH * ap.SH_U and sc.tb == (ap.SH_U // sc.G) * ap.SH_WPH * sc.kpi
        assert sc.S0 in (1, sc.step - 1, sc.step, sc.step + 1, 2 * sc.step + 1) and sc.n in (1, sc.tb - 1, sc.tb, sc.tb + 1)
        assert sc.t_max in (sc.n, 256) and 1 <= sc.n <= sc.t_max and sc.hd % 8 == 0 and sc.S0 + sc.n + 1 < 2 ** sc.bits
    assert [(sc.step, sc.kpi) for sc in ap.SHARED_CASES[::15]] == [(128, 8), (64, 4), (64, 4), (32, 2)]


@pytest.mark.parametrize("dtype,wide", [("bf16", False), ("bf16", True), ("fp32", False), ("fp32", True)])
def test_shared_table_covers_every_pair_of_axes(dtype, wide):
    """Within a template form: every listed value of every axis, each with at least two values of each other axis."""
    cases = [c for c in ap.SHARED_CASES if c.dtype == dtype and (c.hd > 64) == wide]
    assert 0 < len(cases) <= 20 and len(ap.SHARED_CASES) <= 80
    axes = {
        "S0": lambda c: (1, c.step - 1, c.step, c.step + 1, 2 * c.step + 1).index(c.S0),
        "n": lambda c: max(i for i, n in enumerate((1, c.tb - 1, c.tb, c.tb + 1)) if n == c.n),
        "t_max": lambda c: c.t_max == 256,
        "G": lambda c: c.G,
        "hd": lambda c: c.hd,
        "H": lambda c: c.H,
    }
    want = {"S0": 5, "n": 4, "t_max": 2, "G": 5, "hd": 2 if wide else 3, "H": 2}
    assert {c.G for c in cases} == {1, 2, 3, 5, 8} and {c.hd for c in cases} == ({80, 128} if wide else {8, 40, 64}) and {c.H for c in cases} == {4, 5}
    for a, fa in axes.items():
        assert len({fa(c) for c in cases}) == want[a], a
        for value in {fa(c) for c in cases}:
            for b, fb in axes.items():
                if b != a:
                    assert len({fb(c) for c in cases if fa(c) == value}) >= 2, f"{a} = {value} meets one value of {b}"
    assert sorted(c.mask for c in cases if c.mask != "lh") == ["all1", "none"]


@pytest.mark.parametrize("sc", ap.SHARED_CASES, ids=SHARED_IDS)
def test_shared_probes_are_exact_and_read_every_row_key_pair(sc):
    keep = ap.shared_keep(sc)
    case = sc.case
    R, H, Sk, hd, S0 = case.B, case.H, case.Sk, case.hd, sc.S0
    m = ap.shared_mask(sc)
    assert bool(keep[:, 0, 0, S0:].all()) and keep.shape == (R, 1, 1, Sk)
    if m is not None:
        assert m.shape == (sc.B, S0 + 3) and bool((m[:, S0:] == 1).all()) and torch.equal(keep[::sc.G, 0, 0, :S0], m[:, :S0] != 0)
        assert (sc.mask == "all1") == (not m[1, :S0].any())
    g_of = (torch.arange(R) % sc.G).double()
    factor = (1.0 + torch.arange(H, dtype=torch.float64))[None, :, None].repeat(R, 1, Sk)            # [R, H, Sk]
    factor[:, :, S0:] *= (1.0 + g_of)[:, None, None]
    cols, p, picks = [], None, []
    for pr in ap.shared_probes(sc):
        assert all(is_bf16(x) for x in (pr.q, pr.k, pr.v)) and pr.do is None
        assert torch.equal(pr.k[:, :S0], pr.k[::sc.G, :S0].repeat_interleave(sc.G, 0)) and torch.equal(pr.v[:, :S0], pr.v[::sc.G, :S0].repeat_interleave(sc.G, 0))
        buf = ap.shared_buffers(sc, pr)
        assert all(is_bf16(x) for n, x in buf.items() if n != "mask" and x is not None)
        q, k, v, kp = ap.shared_gather(sc, buf)                                                     # the buffers hold the probe, garbage around it
        assert torch.equal(q, pr.q) and torch.equal(k, pr.k) and torch.equal(v, pr.v) and torch.equal(kp, keep)
        assert bool((buf["kp"][:, S0:] == ap.GARBAGE).all()) and bool((buf["vt"][:, sc.n:] == ap.GARBAGE).all()) and bool((buf["kt"][:, sc.n - 1] == -ap.GARBAGE).all())
        ref = ap.reference(pr.q, pr.k, pr.v, None, keep, None, pr.scale)
        if pr.name.startswith("A"):
            assert pr.v.abs().max() <= 40 and not pr.q.any()
            cols.append(ref.val["o"][:, 0])                                                         # [R, H, hd]
            p = ref.p
        else:
            assert bool(((ref.p == 1.0) | (ref.p < 1e-27)).all()) and bool((ref.p.sum(-1) > 0.99).all()) and pr.scale == 1.0
            n_b = int(pr.name[2:-1])
            for r in range(R):
                name = ap.SHARED_PICKS[(r + n_b * R) % len(ap.SHARED_PICKS)]
                t = ap.shared_target(sc, keep[r, 0, 0], name)
                assert bool(keep[r, 0, 0, t]) and bool((ref.p[r, :, 0, t] == 1.0).all())
                picks.append(name)
            assert off_bf16(ref.val["o"]) <= 1e-24
    got = torch.cat(cols, -1)[..., :Sk] / factor
    assert torch.allclose(got, p[:, :, 0], rtol=0, atol=1e-15)                                      # every (row, key) pair in some element
    count = keep.sum(-1, keepdim=True).double()
    assert torch.allclose(p, (keep / count).expand_as(p), rtol=0, atol=1e-15)
    assert set(picks) == set(ap.SHARED_PICKS)                                                       # every pick is asked for in every case


def test_shared_targets_are_the_stated_keys():
    sc = ap.SharedCase("bf16", 2, 4, 257, 5, 256, 64, "lh")
    keep = ap.shared_keep(sc)
    left, holes = keep[0, 0, 0], keep[sc.G, 0, 0]
    assert sc.step == 128 and sc.tb == 64 and left[:257].tolist() == [False] * 5 + [True] * 252
    assert [ap.shared_target(sc, left, p) for p in ap.SHARED_PICKS] == [5, 256, 127, 128, 257, 260, 261]
    vis = torch.nonzero(holes[:257])[:, 0].tolist()
    assert 0.5 < len(vis) / 257 < 0.9 and vis[-1] == 256
    assert [ap.shared_target(sc, holes, p) for p in ap.SHARED_PICKS[:4]] == [vis[0], 256, max(j for j in vis if j <= 127), max(j for j in vis if j <= 128)]
    one = ap.SharedCase("fp32", 3, 5, 1, 1, 1, 80, "all1")
    assert [ap.shared_target(one, ap.shared_keep(one)[0, 0, 0], p) for p in ap.SHARED_PICKS] == [0, 0, 0, 0, 1, 1, 1]
    assert [ap.shared_target(one, ap.shared_keep(one)[3, 0, 0], p) for p in ap.SHARED_PICKS] == [1] * 7       # prompt 1: its tail alone
    assert ap.SharedCase("fp32", 3, 4, 1, 1, 1, 128, "lh").tb == 2 * 2 * 2 and ap.SharedCase("bf16", 5, 4, 1, 1, 1, 8, "lh").tb == 16


@pytest.mark.parametrize("dtype,wide", [("bf16", False), ("bf16", True), ("fp32", False), ("fp32", True)])
def test_shared_emulation_passes_and_every_mutation_is_rejected(dtype, wide):
    """A kernel model that rounds P and the output to the storage type passes every probe of every case of the form.  A model wrong
    in one index (read out of the same buffers) is rejected by some probe of EVERY case in which the mutation changes anything at all,
    and every mutation changes something in at least two cases of the form."""
    rnd = ap._bf16 if dtype == "bf16" else _f32
    hits = {m: 0 for m in ap.SHARED_MUTATIONS}
    worst = 0.0
    for sc in [c for c in ap.SHARED_CASES if c.dtype == dtype and (c.hd > 64) == wide]:
        keep, ok = ap.shared_keep(sc), torch.ones(sc.B * sc.G, 1, dtype=torch.bool)
        truth = [(pr, ap.reference(pr.q, pr.k, pr.v, None, keep, None, pr.scale), ap.shared_buffers(sc, pr)) for pr in ap.shared_probes(sc)]
        right = []
        for pr, ref, buf in truth:
            q, k, v, kp = ap.shared_gather(sc, buf)
            right.append(ap.reference(q, k, v, None, kp, None, pr.scale, rnd=rnd).val["o"])
            worst = max(worst, ap.check({"o": right[-1]}, ref, sc.torch_dtype, ok, pr.exact_zero, what=f"{sc.id} {pr.name}"))
        for mut in ap.SHARED_MUTATIONS:
            altered = rejected = False
            for (pr, ref, buf), good in zip(truth, right):
                q, k, v, kp = ap.shared_gather(sc, buf, mut)
                bad = ap.reference(q, k, v, None, kp, None, pr.scale, rnd=rnd).val["o"]
                altered = altered or not torch.equal(bad, good)
                rejected = rejected or _rejected(lambda: ap.check({"o": bad}, ref, sc.torch_dtype, ok, pr.exact_zero))
            assert rejected == altered, f"{sc.id} {mut}: altered = {altered}, rejected = {rejected}"
            hits[mut] += rejected
    print(f"{dtype} {'wide' if wide else 'narrow'}: worst error / bound of the emulation {worst:.3f}; cases that reject each mutation: {hits}")
    assert 0 < worst <= 1.0 and min(hits.values()) >= 2, hits


# ------------------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("shape", ap.MERGE_CASES, ids=["x".join(map(str, s)) for s in ap.MERGE_CASES])
def test_merge_probe_is_exact_and_rejects_an_index_mix_up(shape):
    B, C, T, H, hd = shape
    rejected = set()
    for pattern in ap.MERGE_PATTERNS:
        o1, o2, l1, l2 = ap.merge_inputs(shape, pattern)
        assert l1.shape == (B, H, C * T) and l2.shape == (B * C, H, T) and l1.dtype == l2.dtype == torch.float32
        assert is_bf16(o1) and is_bf16(o2) and o1.abs().max() <= 8
        want = ap.merge_expected(shape, o1, o2, l1, l2)
        assert is_bf16(want) and torch.equal(ap.merge_emulate(shape, o1, o2, l1, l2), want)
        live = l1[l1 > -1e30]
        assert len(set(live.tolist())) == live.numel()                                              # lse1 differs per (b, h, c, t)
        if pattern == "empty" and B * C * T * H >= 4:
            e1 = (l1 < -1e38).reshape(B, H, C, T).permute(0, 2, 1, 3)
            e2 = (l2 < -1e38).reshape(B, C, H, T)
            assert all(bool(((e1 == a) & (e2 == b)).any()) for a in (False, True) for b in (False, True))
        if pattern == "select":
            assert bool(((l2.reshape(B, C, H, T) - l1.reshape(B, H, C, T).permute(0, 2, 1, 3)).abs() == 200).all())
        for mut in ap.MERGE_MUTATIONS:
            if not torch.equal(ap.merge_emulate(shape, o1, o2, l1, l2, mut), want):
                rejected.add(mut)
    if shape == (1, 1, 1, 1, 8):
        assert not rejected                                                                         # one element: nothing to mix up
    elif C > 1 and T > 1:
        assert rejected == set(ap.MERGE_MUTATIONS)


def test_merge_table_reaches_a_last_partial_workgroup():
    """One thread per 4 columns, 256 threads per workgroup: some case has more than one workgroup and a last one that is not full."""
    assert any(n > 256 and n % 256 for n in [B * C * T * H * hd // 4 for B, C, T, H, hd in ap.MERGE_CASES])


# ------------------------------------------------------------------------------------------------------------------- score flow
@pytest.mark.parametrize("fc", ap.SCORE_FLOW_CASES, ids=[c.id for c in ap.SCORE_FLOW_CASES])
def test_score_flow_probes_and_the_three_roundings_stay_within_the_bound(fc):
    """The float64 flow (two segments merged by their log-sum-exps) equals one attention over the concatenated keys; with o1, o2 and
    the merged output rounded to the storage type it stays inside ap.check's bound as it stands: the worst error / bound of that
    emulation is 0.807 (bf16, 1x2x17, S0 129, hd 80; 0.623 for the S0 65 cases, 0.002 in fp32), so the flow needs no bound of its own."""
    case, keep = fc.case, ap.flow_keep(fc)
    ok = ap.rows_checked(case, keep)
    assert bool(ok.all()) and keep.shape == (fc.B * fc.C, 1, fc.T, fc.S0 + fc.T)
    rnd = ap._bf16 if fc.dtype == "bf16" else _f32
    worst, picks = 0.0, set()
    for pr in ap.flow_probes(fc):
        assert all(is_bf16(x) for x in (pr.q, pr.k, pr.v))
        for x in (pr.k, pr.v):
            assert torch.equal(x[:, :fc.S0], x[::fc.C, :fc.S0].repeat_interleave(fc.C, 0))
        ref = ap.reference(pr.q, pr.k, pr.v, None, keep, None, pr.scale)
        assert torch.allclose(ap.flow_emulate(fc, pr, keep), ref.val["o"], rtol=0, atol=1e-12)
        if pr.name.startswith("B"):
            assert bool(((ref.p == 1.0) | (ref.p < 1e-27)).all())
            picks |= {(int(j) - fc.S0, i) for i in range(fc.T) for j in ref.p[:, 0, i].argmax(-1)}
        worst = max(worst, ap.check({"o": ap.flow_emulate(fc, pr, keep, rnd)}, ref, fc.torch_dtype, ok, pr.exact_zero, what=pr.name))
    print(f"{fc.id}: worst error / bound of the rounded flow {worst:.3f}")
    assert worst <= 1.0
    assert any(j == i for j, i in picks) and any(j == 0 for j, i in picks)                          # the diagonal, the first candidate key
    if fc.masked_prompt is None or fc.B > 1:
        assert any(j == -1 for j, i in picks)                                                       # the last prompt key
