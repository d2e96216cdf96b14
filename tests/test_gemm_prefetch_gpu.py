"""eavqa_gemm_pf (``ops.gemm(..., prefetch=tensor)``): a GEMM that also touches the lines of the weight matrix the NEXT GEMM will stream.

The look-ahead only reads, so every comparison here is bit for bit (``torch.equal``): the same call with and without a region, on every
full-line tile the dispatcher picks from, and a small GPT-2-shaped ``FrozenCausalLM`` through forward + backward with the hints on and off.
One host-only case: the entry point rejects bad arguments before any launch.
"""
import pytest
import torch

DEV = "cuda"

# (M, N, K) on which the dispatcher's cost model (csrc/gemm.hip: k64_cost over K64_AUTO) ranks each of its five full-line tiles first;
# `dispatcher_pick` below is that model, so the list is checked, not trusted
TILE_SHAPES = {"128x80": (1864, 1280, 256), "256x128": (1864, 3840, 256), "256x160": (1864, 5120, 256), "128x128": (1000, 3840, 256),
               "128x256": (546, 11008, 256)}
RAGGED = [(100, 72, 64), (333, 200, 128), (1001, 1288, 192), (130, 3848, 64)]       # M and N off every tile edge (N % 8 == 0: vector rows of C)


def dispatcher_pick(M, N, K):
    tiles = (("128x80", 128, 80, 1.56), ("256x128", 256, 128, 1.97), ("256x160", 256, 160, 1.93), ("128x128", 128, 128, 1.73),
             ("128x256", 128, 256, 1.97))
    cdiv = lambda a, b: (a + b - 1) // b
    best = None
    for name, bm, bn, rate in tiles:
        tm, tn = cdiv(M, bm), cdiv(N, bn)
        gx = min((8, 4, 2, 1), key=lambda g: (cdiv(tm, g) * bm + cdiv(tn, 8 // g) * bn, -g))
        per = cdiv(tm, gx) * cdiv(tn, 8 // gx)
        if cdiv(per, 32) > cdiv(cdiv(tm * tn, 8), 32):
            per = cdiv(tm * tn, 8)
        rounds = cdiv(per, 32)
        cost = rounds * rate * (bm + bn) * (K // 64) + rounds * 0.1 * bm * bn + 4500
        if best is None or cost < best[0]:
            best = (cost, name)
    return best[1]


def test_the_shapes_cover_every_tile_of_the_dispatcher():
    assert {name: dispatcher_pick(*shape) for name, shape in TILE_SHAPES.items()} == {name: name for name in TILE_SHAPES}


def test_gemm_pf_rejects_bad_arguments_before_any_launch():
    """Host only, as eavqa_gemm's own case in test_abi.py: null operands, bad dtype, bad shape, bad alignment - and a negative region size."""
    from eavqa_amd import build, _lib
    build.build()
    lib = _lib.load()
    tail = (None, 0, None, None, 0, None, 0, None)          # bias, act, aux_in, aux_out, ld_aux, residual, ldr, stream
    pf = lib.eavqa_gemm_pf
    assert pf(1, 1, 1, 8, 8, 8, None, 8, None, 8, None, 8, 0, 1.0, *tail, None, 0) == -1
    assert pf(7, 1, 1, 8, 8, 8, 16, 8, 16, 8, 16, 8, 0, 1.0, *tail, None, 0) == -4
    assert pf(1, 1, 1, 8, 8, 12, 16, 16, 16, 16, 16, 8, 0, 1.0, *tail, None, 0) == -3
    assert pf(1, 1, 1, 8, 8, 8, 18, 8, 16, 8, 16, 8, 0, 1.0, *tail, None, 0) == -2
    assert pf(1, 1, 1, 8, 8, 8, 16, 8, 16, 8, 16, 8, 0, 1.0, *tail, 4096, -1) == -1
    assert pf(1, 1, 1, 8, 8, 8, None, 8, None, 8, None, 8, 0, 1.0, *tail, 4096, 1 << 20) == -1    # a region does not excuse null operands


def _regions():
    """Look-ahead regions: a whole matrix, sizes off the 128-byte line, less than a line, nothing, a misaligned start, and a slice that ends
    exactly where its allocation ends (20 MiB: a segment of its own in the caching allocator, so one byte further is not the process's)."""
    big = torch.zeros(20 << 20, dtype=torch.uint8, device=DEV)
    w = torch.randn(1280, 5120, device=DEV).to(torch.bfloat16)
    return {"matrix": w, "odd_size": torch.zeros(128 * 1000 + 77, dtype=torch.uint8, device=DEV), "below_a_line": torch.zeros(100, dtype=torch.uint8, device=DEV),
            "one_line": torch.zeros(128, dtype=torch.uint8, device=DEV), "empty": torch.empty(0, dtype=torch.uint8, device=DEV),
            "misaligned": big[3:3 + 128 * 700 + 5], "end_of_allocation": big[(20 << 20) - 128 * 300 - 50:], "whole_allocation": big}


def _operands(M, N, K, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    b = torch.randn(N, K, device=DEV, generator=g).to(torch.bfloat16)
    return a, b, g


def _epilogues(M, N, g):
    """Keyword sets of ops.gemm: plain, fp32 out, bias + activation + aux_out, activation backward, fp32 / 16-bit residual."""
    bias = torch.randn(N, device=DEV, generator=g)
    res32 = torch.randn(M, N, device=DEV, generator=g)
    u = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    return {"plain": dict(), "out_f32": dict(out_f32=True), "bias_gelu_aux": dict(bias=bias, act="gelu_new", want_aux=True),
            "act_bwd": dict(act="gelu_new", aux_in=u), "bias_res_f32": dict(bias=bias, residual=res32, out_f32=True),
            "res_lowp": dict(bias=bias, residual=res32.to(torch.bfloat16))}


def _run(a, b, kw, prefetch):
    from eavqa_amd import ops
    kw = dict(kw)
    aux = torch.zeros((a.shape[0], b.shape[0]), device=DEV, dtype=a.dtype) if kw.pop("want_aux", False) else None
    out = ops.gemm(a, b, aux_out=aux, prefetch=prefetch, **kw)
    torch.cuda.synchronize()
    return out, aux


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(TILE_SHAPES.values()) + RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_gemm_with_a_region_is_bit_equal_on_every_tile_and_epilogue(shape):
    M, N, K = shape
    a, b, g = _operands(M, N, K)
    region = torch.randn(1280, 5120, device=DEV).to(torch.bfloat16)
    for name, kw in _epilogues(M, N, g).items():
        want, want_aux = _run(a, b, kw, None)
        got, got_aux = _run(a, b, kw, region)
        assert torch.equal(got, want), (shape, name)
        if want_aux is not None:
            assert torch.equal(got_aux, want_aux), (shape, name)
    # the plain result itself is the product (the comparison above would also pass on two equal wrong answers)
    want = a.float() @ b.float().T
    got = _run(a, b, dict(out_f32=True), region)[0]
    assert (got - want).abs().max().item() <= 2e-2 * want.abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", list(TILE_SHAPES))
def test_gemm_is_bit_equal_for_every_kind_of_region(tile):
    M, N, K = TILE_SHAPES[tile]
    a, b, g = _operands(M, N, K, seed=1)
    bias = torch.randn(N, device=DEV, generator=g)
    kw = dict(bias=bias, act="gelu_new", want_aux=True)
    want, want_aux = _run(a, b, kw, None)
    for name, region in _regions().items():
        before = region.clone()
        got, got_aux = _run(a, b, kw, region)
        assert torch.equal(got, want) and torch.equal(got_aux, want_aux), (tile, name)
        assert torch.equal(region, before), (tile, name)               # only read


@pytest.mark.gpu
def test_gemm_region_is_ignored_by_the_kernels_without_a_look_ahead():
    """M <= 64 (the weight-streaming kernel), fp32 and operands that are not k-contiguous take kernels that ignore the region: same bits."""
    region = torch.empty(128 * 999 + 3, dtype=torch.uint8, device=DEV)
    a, b, _ = _operands(32, 512, 256, seed=2)
    assert torch.equal(_run(a, b, {}, region)[0], _run(a, b, {}, None)[0])
    a32, b32 = a.float(), b.float()
    assert torch.equal(_run(a32, b32, {}, region)[0], _run(a32, b32, {}, None)[0])
    a2, b2, _ = _operands(300, 256, 128, seed=3)
    bt = b2.T.contiguous()                                   # [K, N]: Conv1D layout
    assert torch.equal(_run(a2, bt, dict(b_kc=False), region)[0], _run(a2, bt, dict(b_kc=False), None)[0])


@pytest.mark.gpu
def test_prefetch_argument_is_validated():
    from eavqa_amd import ops, _lib
    a, b, _ = _operands(128, 128, 64)
    with pytest.raises(_lib.EavqaError, match="contiguous"):
        ops.gemm(a, b, prefetch=torch.empty(64, 64, device=DEV)[:, :32])
    with pytest.raises(_lib.EavqaError, match="cannot be combined"):
        ops.gemm(a, b, prefetch=b, copy_out=torch.empty(128, 128, device=DEV, dtype=torch.bfloat16))


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [False, True])
def test_frozen_lm_training_step_is_bit_equal_with_and_without_the_hints(pack):
    """A small GPT-2-shaped FrozenCausalLM (more than 64 rows, so its GEMMs take the full-line tiles and not the weight-streaming kernel)
    through forward + backward behind the MLP mapper, packed and padded: loss, logits, the prefix gradient and the mapper's gradients with the
    next-weight hints equal those without, and with the hints every LM GEMM that has a successor goes through eavqa_gemm_pf."""
    import oracle
    from eavqa_amd import ops
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, random_init_state_dict
    E, H, F, NL, V, NPOS = 256, 4, 1024, 3, 512, 64
    cfg = LMConfig("gpt2", NL, H, E, F, V, NPOS, 1e-5, "gelu_new", V - 1, None)
    sd = random_init_state_dict(cfg, 7, "cpu")
    g = torch.Generator().manual_seed(3)
    B, Tt, L, D = 12, 20, 4, 24
    pad = V - 1
    lens = torch.randint(8, Tt + 1, (B,), generator=g)
    ids = torch.randint(2, V - 2, (B, Tt), generator=g)
    mask = (torch.arange(Tt)[None] < lens[:, None]).long()
    ids = ids * mask + pad * (1 - mask)
    labels = oracle.label_mask_cc(ids, pad)
    prefix = torch.randn(B, D, generator=g)
    res = {}
    for hints in (False, True):
        lm = FrozenCausalLM(cfg, sd, torch.bfloat16, DEV)
        assert lm.weight_prefetch                                  # the default for bf16 native weights; EAVQA_WEIGHT_PREFETCH=0 turns it off
        lm.weight_prefetch = hints
        torch.manual_seed(1)
        model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=torch.bfloat16, device=DEV).train()
        model.pack_padding = pack
        seen, dprefix = [], []
        real_call, real_bwd = ops.call, lm.backward
        ops.call = lambda name, *args: (seen.append(name), real_call(name, *args))[1]
        lm.backward = lambda *a, **k: (dprefix.append(real_bwd(*a, **k)), dprefix[-1])[1]
        try:
            out = model(question_tokens=ids, prefix=prefix, question_mask=mask, labels=labels)
            out.loss.backward()
            torch.cuda.synchronize()
        finally:
            ops.call = real_call
        n_pf = sum(n == "eavqa_gemm_pf" for n in seen)
        # forward: four per layer (the last FFN-down names the lm_head); backward: the lm_head dgrad and four per layer but the very last
        assert n_pf == (8 * NL if hints else 0), (hints, n_pf)
        res[hints] = [out.loss.detach().clone(), out.logits.clone(), dprefix[0].clone()] + [p.grad.clone() for p in model.clip_project.parameters()]
    assert len(res[True]) == len(res[False]) > 3
    for x, y in zip(res[False], res[True]):
        assert torch.equal(x, y)
