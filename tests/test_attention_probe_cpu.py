"""The attention probes checked on their own (no GPU): every property tests/_attention_probe.py states of its builders, the bf16
emulation that must pass the acceptance check, and the mutation check - a reference that is wrong by one key (or one bias column)
must be rejected, forward and backward, which is the evidence that the GPU tests would fail on a kernel that is subtly wrong."""
import math

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
