"""GPU: ``eavqa_attention_decode_shared`` (one decode step of B prompts x G rows over ONE prompt cache) against a float64 softmax over
[masked prompt | tail[:t + 1]] computed from the same inputs, and ``eavqa_lm_block_step_shared`` against ``eavqa_lm_block_forward`` on
B * G rows whose prompt caches are repeated G-fold (the tiny GPT-2 / OPT of clipcap_gpt2_mlp.npz / clipcap_opt_mlp.npz)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import _causal_models

DEV = "cuda"
H = 5                  # a 4-head group with a remainder
T = torch.from_numpy

# B, G, hd, S0, t, t_max, mask kind: every value of the issue's lists in at least two combinations
CASES = [
    (1, 1, 64, 1, 0, 6, "ones"), (3, 8, 80, 1, 1, 256, "ones"),
    (3, 3, 80, 63, 1, 6, "left"), (1, 8, 128, 63, 255, 256, "holes"),
    (1, 8, 128, 64, 5, 6, "holes"), (3, 1, 64, 64, 0, 256, "all_masked"),
    (3, 8, 64, 65, 0, 6, "all_masked"), (1, 3, 80, 65, 1, 256, "left"),
    (1, 3, 80, 200, 255, 256, "holes"), (3, 1, 128, 200, 5, 6, "ones"),
    (3, 1, 128, 700, 1, 256, "left"), (3, 3, 64, 700, 5, 6, "all_masked"),
]


def _mask(kind, B, S0, gen):
    m = torch.ones(B, S0 + 2, dtype=torch.int32)           # a row stride that is not S0
    if kind == "left":
        for b in range(B):
            m[b, :(b * S0) // (B + 1)] = 0
    elif kind == "holes":
        m[:, :S0] = (torch.rand(B, S0, generator=gen) > 0.35).to(torch.int32)
    elif kind == "all_masked":                              # one prompt with EVERY key masked: its rows see their tail alone
        m[:, :S0] = (torch.rand(B, S0, generator=gen) > 0.2).to(torch.int32)
        m[B // 2, :S0] = 0
    return m


def _inputs(B, G, hd, S0, t, t_max, kind, dtype, twins=False, seed=0):
    gen = torch.Generator().manual_seed(seed + 31 * S0 + G)
    E, R, pbr = H * hd, B * G, S0 + 3
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dtype)
    qkv = rnd(R, 3 * E)                                     # q | k_new | v_new as the QKV projection leaves them
    kp, vp = rnd(B, pbr, E), rnd(B, pbr, E)
    kt, vt = rnd(R, t_max, E), rnd(R, t_max, E)
    if twins:                                               # the rows of a prompt: one q, one tail
        first = lambda x: x.view(B, G, *x.shape[1:])[:, :1].expand(B, G, *x.shape[1:]).reshape(x.shape).clone()
        qkv, kt, vt = first(qkv), first(kt), first(vt)
    return dict(qkv=qkv, kp=kp, vp=vp, kt=kt, vt=vt, mask=_mask(kind, B, S0, gen))


def _reference(x, B, G, hd, S0, t):
    """float64 [B * G, H * hd]: softmax over [masked prompt keys | tail 0..t-1 | the new key] per row and head."""
    E, R = H * hd, B * G
    d = lambda a: a.double()
    q, kn, vn = (d(x["qkv"][:, i * E:(i + 1) * E]).view(B, G, H, hd) for i in range(3))
    kp, vp = d(x["kp"][:, :S0]).view(B, S0, H, hd), d(x["vp"][:, :S0]).view(B, S0, H, hd)
    kt = torch.cat([d(x["kt"][:, :t]).view(B, G, t, H, hd), kn[:, :, None]], dim=2)
    vt = torch.cat([d(x["vt"][:, :t]).view(B, G, t, H, hd), vn[:, :, None]], dim=2)
    sp = torch.einsum("bghd,bshd->bghs", q, kp) * hd ** -0.5
    sp = sp.masked_fill(x["mask"][:, None, None, :S0] == 0, float("-inf"))
    stl = torch.einsum("bghd,bgihd->bghi", q, kt) * hd ** -0.5
    p = torch.softmax(torch.cat([sp, stl], dim=-1), dim=-1)
    out = torch.einsum("bghs,bshd->bghd", p[..., :S0], vp) + torch.einsum("bghi,bgihd->bghd", p[..., S0:], vt)
    vmax = max(float(vp.abs().max()), float(vt.abs().max()))
    return out.reshape(R, E), vmax


def _run(x, B, G, hd, S0, t):
    from eavqa_amd import ops
    E = H * hd
    g = {k: v.to(DEV) for k, v in x.items()}
    before = {k: g[k].clone() for k in ("kp", "vp", "kt", "vt")}
    pbr = g["kp"].shape[1]
    out = ops.attention_decode_shared(g["qkv"][:, :E], g["kp"].view(B * pbr, E), g["vp"].view(B * pbr, E), g["kt"], g["vt"], g["qkv"][:, E:2 * E],
                                      g["qkv"][:, 2 * E:], B, G, H, S0, t, hd, prompt_batch_rows=pbr, key_mask=g["mask"],
                                      ld_mask=g["mask"].stride(0), scale=hd ** -0.5)
    torch.cuda.synchronize()
    return out, g, before


def _bound(dtype, vmax):
    # fp32: the project's fp32 step bound (tests/test_beam_gpu.py).  bf16: the output is a convex combination of V rows rounded once to
    # bf16 - half an ulp is 2^-9 relative, doubled for the fp32 summation order.
    return 1e-5 * max(1.0, vmax) if dtype == torch.float32 else 2.0 ** -8 * vmax


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-G{c[1]}-hd{c[2]}-S{c[3]}-t{c[4]}of{c[5]}-{c[6]}" for c in CASES])
def test_kernel_matches_a_float64_softmax_over_prompt_and_tail(case, dtype):
    B, G, hd, S0, t, t_max, kind = case
    x = _inputs(B, G, hd, S0, t, t_max, kind, dtype)
    want, vmax = _reference(x, B, G, hd, S0, t)
    out, g, before = _run(x, B, G, hd, S0, t)
    E = H * hd
    err = float((out.double().cpu() - want).abs().max())
    print(f"[{case} {dtype}] max |out - float64| {err:.3e} (bound {_bound(dtype, vmax):.3e})")
    assert out.dtype == dtype and torch.isfinite(out.float()).all()
    assert err <= _bound(dtype, vmax)
    # the new position was appended bit for bit, nothing else moved
    assert torch.equal(g["kt"][:, t], g["qkv"][:, E:2 * E]) and torch.equal(g["vt"][:, t], g["qkv"][:, 2 * E:])
    keep = torch.ones(t_max, dtype=torch.bool, device=DEV)
    keep[t] = False
    assert torch.equal(g["kt"][:, keep], before["kt"][:, keep]) and torch.equal(g["vt"][:, keep], before["vt"][:, keep])
    assert torch.equal(g["kp"], before["kp"]) and torch.equal(g["vp"], before["vp"])
    if kind == "all_masked":                                # the fully masked prompt's rows are their tail's softmax alone
        sl = slice((B // 2) * G, (B // 2 + 1) * G)
        tail_only = _tail_only({k: x[k][sl] for k in ("qkv", "kt", "vt")}, G, hd, t)
        assert float((out[sl].double().cpu() - tail_only).abs().max()) <= _bound(dtype, vmax)


def _tail_only(x, G, hd, t):
    E = H * hd
    d = lambda a: a.double()
    q, kn, vn = (d(x["qkv"][:, i * E:(i + 1) * E]).view(G, H, hd) for i in range(3))
    kt = torch.cat([d(x["kt"][:, :t]).view(G, t, H, hd), kn[:, None]], dim=1)
    vt = torch.cat([d(x["vt"][:, :t]).view(G, t, H, hd), vn[:, None]], dim=1)
    p = torch.softmax(torch.einsum("ghd,gihd->ghi", q, kt) * hd ** -0.5, dim=-1)
    return torch.einsum("ghi,gihd->ghd", p, vt).reshape(G, E)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(3, 3, 80, 65, 5, 6, "holes"), (1, 8, 64, 200, 0, 6, "left"), (3, 8, 128, 63, 40, 256, "ones"),
                                  (1, 5, 80, 64, 9, 256, "holes")], ids=lambda c: f"G{c[1]}-hd{c[2]}-S{c[3]}-t{c[4]}")
def test_rows_of_a_prompt_with_one_q_and_one_tail_come_out_identical(case, dtype):
    B, G, hd, S0, t, t_max, kind = case
    x = _inputs(B, G, hd, S0, t, t_max, kind, dtype, twins=True)
    out, _, _ = _run(x, B, G, hd, S0, t)
    rows = out.view(B, G, -1)
    assert torch.equal(rows, rows[:, :1].expand_as(rows))
    want, vmax = _reference(x, B, G, hd, S0, t)
    assert float((out.double().cpu() - want).abs().max()) <= _bound(dtype, vmax)


REJECTIONS = [(dict(G=9), -3), (dict(t=6), -1), (dict(hd=132), -3), (dict(S0=3585), -3), (dict(q=None), -1), (dict(k_tail=None), -1),
              (dict(dtype=7), -4), (dict(t_max=257, t=0), -3), (dict(ld_tail=12), -2)]


@pytest.mark.parametrize("fault,code", REJECTIONS, ids=["-".join(f"{k}_{v}" for k, v in f.items()) for f, _ in REJECTIONS])
def test_rejections_come_before_any_launch(fault, code):
    """16 stands for an aligned pointer that is never dereferenced: a call that reached a launch would fault."""
    from eavqa_amd import _lib
    a = dict(dtype=1, B=1, G=2, H=1, S0=4, t=1, t_max=6, hd=8, q=16, ldq=8, k_prompt=16, ldk=8, v_prompt=16, ldv=8, prompt_batch_rows=4,
             k_tail=16, v_tail=16, ld_tail=8, k_new=16, v_new=16, ld_new=8, o=16, ldo=8, key_mask=None, ld_mask=0, scale=1.0, stream=None)
    assert not set(fault) - set(a)
    a.update(fault)
    assert _lib.load().eavqa_attention_decode_shared(*a.values()) == code


# ------------------------------------------------------------------------------------------------ the block step
def _one_layer(table, l, kind):
    one = (kind * 1)()
    C.memmove(one, C.byref(table[l]), C.sizeof(kind))
    return one


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_block_step_equals_the_plain_step_on_repeated_prompt_caches(arch, dtype):
    """B = 2 prompts (one padded), G = 3 rows each, two tail positions already there.  The whole stack: the residual streams agree within
    the bounds of test_beams_decoder_step_equals_the_plain_step_on_repeated_encoder_outputs.  The appended K / V rows: bit for bit, checked
    layer by layer with ONE input per layer - behind layer 0 the two routes' inputs differ by their attention kernels' summation order, so
    equality of later layers' rows in a stacked run would be luck, not a property."""
    from eavqa_amd import _lib, ops
    from eavqa_amd.models import decode
    z, model = _causal_models.model(arch, dtype)
    lm = model.gpt
    B, G, t, t_max = 2, 3, 2, 4
    R, E, nl = B * G, lm.cfg.n_embd, len(lm.layers)
    assert (z["gen_mask"][1] == 0).any()
    rows, src, mask, pos, _, S0 = model._plain_prompt(T(z["gen_ids"][:2]), T(z["prefix"][:2]), T(z["gen_mask"][:2]), t_max)
    drv = decode._SharedStep(lm, B, G, S0, t_max, 1)
    drv.prefill(rows, src, pos, mask)
    gen = torch.Generator().manual_seed(5)
    drv.planes[0].copy_((0.5 * torch.randn(drv.planes[0].shape, generator=gen)).to(dtype))
    S_max = S0 + t_max
    rep = decode._KVCache(lm, R, S_max, R)
    for l in range(nl):
        for shared, tail, full in ((drv.cache.k[l], drv.planes[0][2 * l], rep.k[l]), (drv.cache.v[l], drv.planes[0][2 * l + 1], rep.v[l])):
            f = full.view(R, S_max, E)
            f[:, :S0] = shared.view(B, S0, E).repeat_interleave(G, dim=0)
            f[:, S0:] = tail
    mask_r = mask.repeat_interleave(G, dim=0).contiguous()
    x0 = torch.randn(R, E, generator=gen).to(DEV)
    did = ops.dtype_id(dtype)
    c = lm.cfg

    def shared_step(x, layers, tails, n):
        _lib.call("eavqa_lm_block_step_shared", did, n, layers, tails, E, c.n_head, c.ffn, _lib.ACT[c.act], float(c.eps), B, G, S0, S0, t, t_max,
                  x.data_ptr(), mask.data_ptr(), mask.stride(0), drv.ws.data_ptr(), drv.ws_bytes, ops._stream())

    def plain_step(x, layers, n):
        _lib.call("eavqa_lm_block_forward", did, n, layers, E, c.n_head, c.ffn, _lib.ACT[c.act], float(c.eps), R, 1, S0 + t, S_max, x.data_ptr(),
                  mask_r.data_ptr(), mask_r.stride(0), rep.ws.data_ptr(), rep.ws_bytes, ops._stream())

    for l in range(nl):                                     # every layer from the same input: the appended rows are bit-identical
        got, want = x0.clone(), x0.clone()
        shared_step(got, _one_layer(drv.cache.table, l, _lib.LMLayer), _one_layer(drv.tails[0], l, _lib.LMTail), 1)
        plain_step(want, _one_layer(rep.table, l, _lib.LMLayer), 1)
        torch.cuda.synchronize()
        for plane, full in ((drv.planes[0][2 * l], rep.k[l]), (drv.planes[0][2 * l + 1], rep.v[l])):
            assert torch.equal(plane[:, t], full.view(R, S_max, E)[:, S0 + t]), f"layer {l}"
            assert torch.equal(plane[:, :t], full.view(R, S_max, E)[:, S0:S0 + t])
    got, want = x0.clone(), x0.clone()
    shared_step(got, drv.cache.table, drv.tails[0], nl)
    plain_step(want, rep.table, nl)
    torch.cuda.synchronize()
    err = float((got - want).abs().max())
    bound = 1e-5 if dtype == torch.float32 else 6e-2 * max(1.0, float(want.abs().max()))
    print(f"[{arch} {dtype}] block step: max |shared - replicated| {err:.3e} (bound {bound:.3e})")
    assert torch.isfinite(got).all() and err <= bound
    assert torch.equal(drv.planes[0][0][:, t], rep.k[0].view(R, S_max, E)[:, S0 + t])       # layer 0 of the stacked run as well
