"""GPU: training on interleaved image-text rows on both LM families - ``ops.build_fewshot_labels``, ``ClipCaptionModel.forward_fewshot``,
``VCT0Model.forward`` with text, the transformer mapper on several images per row, the executors.

References: tests/_incontext_ref.py (label layout, and the oracle composition with autograd) and tests/golden/incontext.npz (the reference's
code + HF).  Causal tolerances are ``TOL`` of tests/test_model_gpu.py, T5 tolerances those of ``test_vct0_training_step_matches_reference``
(tests/test_t5_gpu.py), restated in ``T5_TOL``."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _incontext_ref as ref
from _metrics import grad_stats
from conftest import load_golden
from test_model_gpu import TOL, _tiny_lm, build_model

DEV = "cuda"
T = torch.from_numpy
# tests/test_t5_gpu.py::test_vct0_training_step_matches_reference: |d loss| <= tol, logits <= tol * max(1, max |want|), gradient statistics
T5_TOL = {torch.float32: dict(tol=2e-4, maxrel=1e-3, cos=0.999999, ratio=1e-4), torch.bfloat16: dict(tol=6e-2, maxrel=0.15, cos=0.995, ratio=2e-2)}
FIXTURES = {("gpt2", "mlp"): "clipcap_gpt2_mlp.npz", ("gpt2", "transformer"): "clipcap_gpt2_transformer.npz", ("opt", "mlp"): "clipcap_opt_mlp.npz"}


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.clip_project.named_parameters()}


def reset(model):
    model.clip_project.zero_grad(set_to_none=True)


def check_grad_stats(tag, got, want, dtype):
    b = T5_TOL[dtype]
    cos, ratio, maxrel = grad_stats({k: v.float().cpu() for k, v in got.items()}, want)
    print(f"[{tag} {dtype}] gradient cosine {cos:.6f}  norm ratio {ratio:.5f}  max rel {maxrel:.2e}")
    assert maxrel <= b["maxrel"] and cos >= b["cos"] and abs(ratio - 1) <= b["ratio"], (tag, cos, ratio, maxrel)


# ================================================================================================ 1. the label layout
def _label_rows(T_, n_img, special):
    """Rows of T_ tokens that put sentinels on the places the walk can get wrong: position 0, 63 | 64 (the carry between two 64-token
    passes), T_ - 1, two adjacent ones; a label on a sentinel; right padding; a row with too few sentinels and (n_img > 1) one with
    too many."""
    g = torch.Generator().manual_seed(100 * T_ + n_img)
    spots = [[0, 63, 64], [63, 64, T_ - 1], [0, 1, T_ - 1], [5, 64, 65], [T_ - 3, T_ - 2, T_ - 1], [64, 66, 68]]
    B = len(spots) + 2
    tok = torch.randint(3, special - n_img - 1, (B, T_), generator=g)
    labels = torch.randint(3, special - n_img - 1, (B, T_), generator=g)
    labels[torch.rand(B, T_, generator=g) < 0.4] = -100
    for b, s in enumerate(spots):
        for i, p in enumerate(s[:n_img]):
            tok[b, p] = special - i
            labels[b, p] = 11 + i                               # a label ON a sentinel: must come out -100
    labels[1, 40:] = -100                                       # a padded row keeps -100 behind its end (sentinels there still expand)
    labels[3, T_ - 6:] = -100
    if n_img > 1:
        tok[B - 2, 10] = special                                # too few: one sentinel of n_img
        tok[B - 1, [2, 3, 64, 65]] = torch.tensor([special, special - 1, special, special - 1])      # too many: four
    return tok, labels                                          # (n_img == 1: rows B-2 / B-1 hold no sentinel at all: too few)


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("n_img", [1, 3])
def test_label_layout_is_exact(ops, L, n_img):
    T_, special = 70, 90
    tok, labels = _label_rows(T_, n_img, special)
    want, want_scored = ref.expand_labels(tok.numpy(), labels.numpy(), L, n_img, special)
    out, scored = ops.build_fewshot_labels(tok.to(DEV), labels.to(DEV), L, n_img, special)
    assert out.dtype == torch.int64 and tuple(out.shape) == (tok.shape[0], T_ + (L - 1) * n_img) and scored.dtype == torch.int32
    assert np.array_equal(out.cpu().numpy(), want)
    assert scored.cpu().tolist() == want_scored.tolist()
    # the labels sit where eavqa_build_fewshot_rows put their tokens, on every row that holds its n_img sentinels
    src, _, _, status = ops.build_fewshot_rows(tok.to(DEV), torch.ones_like(tok).to(DEV), L, n_img, special, 0)
    ok = (status == n_img).cpu()
    assert int(ok.sum()) == 6
    lab_tok = torch.where(labels != -100, tok, torch.full_like(tok, -100))                 # label := the token itself
    lab_tok[ref.is_sentinel(tok.numpy(), n_img, special)] = -100
    moved, _ = ops.build_fewshot_labels(tok.to(DEV), lab_tok.to(DEV), L, n_img, special)
    same = (moved.cpu() == -100) | (moved.cpu() == src.cpu())
    assert bool(same[ok].all())


def test_label_layout_row_bound_and_arguments(ops):
    from eavqa_amd import _lib
    L, n_img, special = 2, 1, 7
    T_ok = 60 * 1024 // 4 - (L - 1) * n_img                     # the longest row eavqa_build_fewshot_rows accepts
    tok = torch.randint(8, 50, (1, T_ok + 1))
    tok[0, 12345] = special
    labels = tok.clone()
    labels[0, ::3] = -100
    tk, lb = tok.to(DEV), labels.to(DEV)
    with pytest.raises(_lib.EavqaError, match=rf"\(code {_lib.EAVQA_E_SHAPE}\)"):        # past the 60 KiB row: the bound of the rows themselves
        ops.build_fewshot_labels(tk, lb, L, n_img, special)
    with pytest.raises(_lib.EavqaError, match=rf"\(code {_lib.EAVQA_E_SHAPE}\)"):
        ops.build_fewshot_rows(tk, torch.ones_like(tk), L, n_img, special, 0)
    # the longest accepted row: 240 passes of the scan
    got, n = ops.build_fewshot_labels(tk[:, :T_ok].contiguous(), lb[:, :T_ok].contiguous(), L, n_img, special)
    want, want_n = ref.expand_labels(tok[:, :T_ok].numpy(), labels[:, :T_ok].numpy(), L, n_img, special)
    assert np.array_equal(got.cpu().numpy(), want) and n.cpu().tolist() == want_n.tolist()
    with pytest.raises(ValueError, match="labels"):
        ops.build_fewshot_labels(tk, lb[:, :5], L, n_img, special)
    with pytest.raises(ValueError, match="special_token_id"):
        ops.build_fewshot_labels(tk, lb, L, n_img, -1)
    with pytest.raises(_lib.EavqaError, match="no CPU fallback"):
        ops.build_fewshot_labels(tok, labels, L, n_img, special)


# ================================================================================================ 2. bit equality with what exists
def _free_id(ids, V):
    used = set(np.asarray(ids).flatten().tolist())
    return next(v for v in range(V - 2, 2, -1) if v not in used)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pack", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("arch,mapping_type", list(FIXTURES))
def test_forward_fewshot_with_one_leading_image_is_forward_bit_for_bit(arch, mapping_type, pack, dtype):
    """One image per row and the sentinel as first token is the row ``forward`` builds: the two paths must issue identical work.
    (The transformer mapper's LayerNorm parameter gradients are float atomics, one per 64 rows and column: with B * (clip_length + L) <=
    128 rows at most two terms meet in a column, and their sum does not depend on the order.)"""
    z = load_golden(FIXTURES[(arch, mapping_type)])
    model = build_model(z, arch, mapping_type, dtype).train()
    model.pack_padding = pack
    if mapping_type == "transformer":
        assert z["ids"].shape[0] * (model.clip_project.clip_length + model.prefix_length) <= 128
    ids, mask, labels, prefix = T(z["ids"]), T(z["mask"]), T(z["labels"]), T(z["prefix"])
    B, L = ids.shape[0], model.prefix_length
    special = _free_id(z["ids"], int(z["cfg"][0]))
    a = model(question_tokens=ids, prefix=prefix, question_mask=mask, labels=labels)
    a.loss.backward()
    ga, la = grads_of(model), a.logits.clone()
    reset(model)
    col = lambda v: torch.full((B, 1), v, dtype=torch.long)
    b = model.forward_fewshot(torch.cat([col(special), ids], 1), prefix[:, None], torch.cat([col(1), mask], 1), torch.cat([col(-100), labels], 1),
                              num_shots=0, special_token_id=special)
    b.loss.backward()
    gb = grads_of(model)
    reset(model)
    assert torch.equal(a.loss, b.loss)
    assert tuple(b.logits.shape) == tuple(la.shape)
    attended = torch.cat([torch.ones(B, L, dtype=torch.bool), mask != 0], 1).to(DEV)
    assert torch.equal(la[attended], b.logits[attended])
    if pack:
        assert bool((b.logits[~attended] == 0).all())
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # without labels: the logits of every position, as forward
    model.eval()
    assert torch.equal(model(question_tokens=ids, prefix=prefix, question_mask=mask).logits,
                       model.forward_fewshot(torch.cat([col(special), ids], 1), prefix[:, None], torch.cat([col(1), mask], 1), special_token_id=special).logits)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_t5_forward_with_a_lone_sentinel_is_the_caption_step_bit_for_bit(dtype):
    from test_t5_gpu import _model
    z, T_, model, V = _model("t0", dtype)
    prefix, labels = T_(z["prefix"]), T_(z["labels"])
    B = prefix.shape[0]
    a = model(prefix=prefix, labels=labels)
    a.loss.backward()
    ga = grads_of(model)
    reset(model)
    b = model(prefix=prefix, labels=labels, question_tokens=torch.full((B, 1), V - 1), question_mask=torch.ones(B, 1, dtype=torch.long),
              special_token_id=V - 1)
    b.loss.backward()
    gb = grads_of(model)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.logits, b.logits)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("arch", ["gpt2", "opt"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_packed_forward_fewshot_ignores_appended_pad_columns(arch, dtype):
    z = load_golden(FIXTURES[(arch, "mlp")])
    f = load_golden("incontext.npz")
    model = build_model(z, arch, "mlp", dtype).train()
    _, tok, mask, prefix, labels, special = ref.fixture_cases(f, arch)[1]
    B = tok.shape[0]
    a = model.forward_fewshot(tok, prefix, mask, labels, special_token_id=special)
    a.loss.backward()
    ga = grads_of(model)
    reset(model)
    pad = lambda t, v: torch.cat([t, torch.full((B, 5), v, dtype=t.dtype)], 1)
    b = model.forward_fewshot(pad(tok, int(z["pad_id"])), prefix, pad(mask, 0), pad(labels, -100), special_token_id=special)
    b.loss.backward()
    gb = grads_of(model)
    assert torch.equal(a.loss, b.loss)
    assert torch.equal(a.logits, b.logits[:, :a.logits.shape[1]]) and bool((b.logits[:, a.logits.shape[1]:] == 0).all())
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


# ================================================================================================ 3. against the fixture
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pack", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_forward_fewshot_matches_the_reference_fixture(arch, pack, dtype):
    z, f = load_golden(FIXTURES[(arch, "mlp")]), load_golden("incontext.npz")
    model = build_model(z, arch, "mlp", dtype).train()
    model.pack_padding = pack
    tol = TOL[dtype]
    for name, tok, mask, prefix, labels, special in ref.fixture_cases(f, arch):
        out = model.forward_fewshot(tok, prefix, mask, labels, num_shots=2, special_token_id=special)
        want = T(f[f"{arch}.logits"])
        assert tuple(out.logits.shape) == tuple(want.shape)
        attended = ref.expanded_mask(tok, mask, model.prefix_length, 3, special)
        diff = (out.logits.float().cpu() - want).abs()
        if pack:
            assert bool((out.logits.cpu()[~attended] == 0).all())
            diff = diff[attended]
        d_loss = abs(out.loss.item() - float(f[f"{arch}.{name}.loss"]))
        print(f"[{arch} {name} {dtype} pack={pack}] |d loss| {d_loss:.2e}  max |d logits| {diff.max().item():.2e}")
        assert diff.max().item() <= tol["logits"] and d_loss <= tol["loss"]
        out.loss.backward()
        for k, p in model.clip_project.named_parameters():
            g = T(f[f"{arch}.{name}.gmap.{k}"])
            err = (p.grad.float().cpu() - g).abs().max().item()
            assert err <= tol["grad"] * max(1.0, g.abs().max().item()), (name, k, err)
        reset(model)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_vct0_forward_with_text_matches_the_reference_fixture(dtype):
    from test_t5_gpu import _model
    f = load_golden("incontext.npz")
    z, T_, model, V = _model("t0", dtype)
    b = T5_TOL[dtype]
    for name, tok, mask, prefix, labels, special in ref.fixture_cases(f, "t0"):
        out = model(prefix=prefix, labels=labels, question_tokens=tok, question_mask=mask, num_shots=2, special_token_id=special)
        want = T(f[f"t0.{name}.logits"])
        d_loss = abs(out.loss.item() - float(f[f"t0.{name}.loss"]))
        d_logits = (out.logits.float().cpu() - want).abs().max().item()
        print(f"[t0 {name} {dtype}] |d loss| {d_loss:.2e}  max |d logits| {d_logits:.2e} (max |logit| {want.abs().max().item():.1f})")
        assert d_loss <= b["tol"] and d_logits <= b["tol"] * max(1.0, want.abs().max().item())
        out.loss.backward()
        check_grad_stats(f"t0 {name}", grads_of(model), {k: T(f[f"t0.{name}.gmap.{k}"]) for k, _ in model.clip_project.named_parameters()}, dtype)
        reset(model)


# ================================================================================================ 4. head dim 64, two attention tiles
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pack", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_forward_fewshot_beyond_one_attention_tile_on_head_dim_64(arch, pack, dtype):
    """E = 128, 2 heads (head dim 64: the matrix-core attention routes), T = 70 -> T' = 76 (two tiles), rows attending 76, 40 and 9 positions,
    prefix rows in the middle of the packed causal rows."""
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM
    cfg, sd = _tiny_lm(V=96, E=128, n_layer=2, n_head=2, arch=arch)
    L, D, n_img, special = 3, 16, 3, 96 - 5
    lm = FrozenCausalLM(cfg, sd, dtype, DEV)
    torch.manual_seed(1)
    model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=DEV).train()
    model.pack_padding = pack
    tok, mask, labels = ref.long_episode(96, special, L=L, n_img=n_img)
    prefix = torch.randn(3, n_img, D, generator=torch.Generator().manual_seed(2))
    attended = ref.expanded_mask(tok, mask, L, n_img, special)
    assert attended.shape[1] == 76 and attended.sum(1).tolist() == [76, 40, 9]
    out = model.forward_fewshot(tok, prefix, mask, labels, special_token_id=special)
    out.loss.backward()
    mapper = {k: v.detach().float().cpu() for k, v in model.clip_project.state_dict().items()}
    ocfg = dict(arch=arch, n_layer=cfg.n_layer, n_head=cfg.n_head, act=cfg.act)
    loss, logits, want, _ = ref.causal_oracle(sd, ocfg, mapper, dict(prefix_length=L, mapping_type="mlp"), tok, prefix, mask, labels, n_img, special)
    tol = TOL[dtype]
    d_loss = abs(out.loss.item() - loss.item())
    d_logits = (out.logits.float().cpu()[attended] - logits.float()[attended]).abs().max().item()
    print(f"[{arch} hd64 {dtype} pack={pack}] |d loss| {d_loss:.2e}  max |d logits| {d_logits:.2e}")
    assert d_loss <= tol["loss"]
    got = grads_of(model)
    if dtype == torch.float32:
        assert d_logits <= tol["logits"]
        for k, g in want.items():
            assert (got[k].cpu() - g.float()).abs().max().item() <= tol["grad"] * max(1.0, g.abs().max().item()), k
    check_grad_stats(f"{arch} hd64 pack={pack}", got, want, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_vct0_forward_with_text_beyond_one_attention_tile_on_head_dim_64(dtype):
    """d_model 128, d_kv 64, 2 heads, gated, 2 + 2 layers: the encoder runs 76 positions (two tiles) under a padding mask, the cross-attention
    sees 76 keys of which rows 1 and 2 mask 36 and 67."""
    from eavqa_amd.models.t5 import FrozenT5, T5Config, random_init_t5_state_dict
    from eavqa_amd.models.vct0 import VCT0Prefix
    V, L, D, n_img = 96, 3, 16, 3
    cfg = T5Config(128, 64, 2, 256, 2, 2, V, True, False)
    sd = random_init_t5_state_dict(cfg, 5, "cpu")
    lm = FrozenT5(cfg, sd, dtype, DEV)
    torch.manual_seed(1)
    model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=DEV).train()
    special = V - 1
    tok, mask, _ = ref.long_episode(V, special, L=L, n_img=n_img)
    g = torch.Generator().manual_seed(3)
    prefix = torch.randn(3, n_img, D, generator=g)
    labels = torch.randint(2, V - 8, (3, 7), generator=g)
    labels[1, 5:] = -100
    labels[2, 3:] = -100
    out = model(prefix=prefix, labels=labels, question_tokens=tok, question_mask=mask, special_token_id=special)
    out.loss.backward()
    mapper = {k: v.detach().float().cpu() for k, v in model.clip_project.state_dict().items()}
    ocfg = dict(n_layer=2, n_dec_layer=2, n_head=2, d_kv=64, gated=True, tied=False)
    loss, logits, want = ref.t5_oracle(sd, ocfg, mapper, dict(prefix_length=L, mapping_type="mlp"), tok, prefix, mask, labels, n_img, special)
    b = T5_TOL[dtype]
    d_loss = abs(out.loss.item() - loss.item())
    d_logits = (out.logits.float().cpu() - logits.float()).abs().max().item()
    print(f"[t5 hd64 {dtype}] |d loss| {d_loss:.2e}  max |d logits| {d_logits:.2e} (max |logit| {logits.abs().max().item():.1f})")
    assert d_loss <= b["tol"] and d_logits <= b["tol"] * max(1.0, logits.abs().max().item())
    check_grad_stats("t5 hd64", grads_of(model), want, dtype)


# ================================================================================================ 5. transformer mapper, several images
def test_transformer_mapper_with_several_images_per_row():
    """``generate_fewshot`` ids (fp32, exact) and ``forward_fewshot`` loss / logits / gradients against the oracle on the transformer-mapper
    fixture's weights: the mapper takes the B * n_img images as its batch."""
    z = load_golden(FIXTURES[("gpt2", "transformer")])
    sd, ocfg, mapper, mcfg = ref.causal_pieces(z, "gpt2", "transformer")
    V, D, L = int(z["cfg"][0]), int(z["cfg"][6]), mcfg["prefix_length"]
    special = V - 5
    tok, mask, last, every = ref.episode(V, special)
    prefix = torch.randn(3, 3, D, generator=torch.Generator().manual_seed(4))
    model = build_model(z, "gpt2", "transformer", torch.float32).eval()
    pad = int(z["pad_id"])
    # the few-shot greedy loop of tests/test_model_gpu.py (eos None) behind the transformer mapper's projections
    import oracle
    pp = oracle.mapper_project(prefix.reshape(9, D), mapper, "transformer", L, int(z["cfg"][1]), mcfg["clip_length"], mcfg["num_layers"])
    wte = sd["transformer.wte.weight"]
    with torch.no_grad():
        emb, am = oracle.insert_prefix_into_input(L, 2, tok, wte[tok], pp.reshape(3, 3, L, -1), mask, special_token_id=special)
        want_ids = []
        am = am.float()
        for _ in range(5):
            nxt = oracle.lm_logits(sd, ocfg, emb, am)[:, -1].argmax(-1, keepdim=True)
            want_ids.append(nxt)
            emb, am = torch.cat([emb, wte[nxt]], 1), torch.cat([am, torch.ones(3, 1)], 1)
    got = model.generate_fewshot(tok, prefix, mask, num_shots=2, special_token_id=special, max_length=5, pad_token_id=pad, eos_token_id=None)
    assert got == torch.cat(want_ids, 1).tolist()
    model.train()
    tol = TOL[torch.float32]
    for labels in (last, every):
        out = model.forward_fewshot(tok, prefix, mask, labels, special_token_id=special)
        out.loss.backward()
        loss, logits, want, _ = ref.causal_oracle(sd, ocfg, mapper, mcfg, tok, prefix, mask, labels, 3, special)
        attended = ref.expanded_mask(tok, mask, L, 3, special)
        assert abs(out.loss.item() - loss.item()) <= tol["loss"]
        assert (out.logits.cpu()[attended] - logits.float()[attended]).abs().max().item() <= tol["logits"]
        got_g = grads_of(model)
        for k, g in want.items():
            assert (got_g[k].cpu() - g.float()).abs().max().item() <= tol["grad"] * max(1.0, g.abs().max().item()), k
        reset(model)


def test_forward_fewshot_rejects_a_wrong_sentinel_count_on_host_and_device_tensors():
    z = load_golden(FIXTURES[("gpt2", "mlp")])
    model = build_model(z, "gpt2", "mlp", torch.float32).train()
    V, D = int(z["cfg"][0]), int(z["cfg"][6])
    tok, mask, last, _ = ref.episode(V, V - 5)
    bad = tok.clone()
    bad[2, ref.is_sentinel(tok.numpy(), 3, V - 5)[2].argmax()] = 3
    prefix = torch.randn(3, 3, D)
    for move in (lambda t: t, lambda t: t.to(DEV)):
        with pytest.raises(ValueError, match="every row must hold exactly one sentinel token per image"):
            model.forward_fewshot(move(bad), prefix, move(mask), move(last), special_token_id=V - 5)
    with pytest.raises(ValueError, match="num_shots"):
        model.forward_fewshot(tok, prefix, mask, last, num_shots=4, special_token_id=V - 5)
    # device tensors: lengths and the label count are left to the device (every packed row goes through the lm_head, so the mean over
    # the scored rows is taken in another order: equal to rounding, not to the bit)
    a = model.forward_fewshot(tok, prefix, mask, last, special_token_id=V - 5).loss
    b = model.forward_fewshot(tok.to(DEV), prefix.to(DEV), mask.to(DEV), last.to(DEV), special_token_id=V - 5).loss
    assert abs(a.item() - b.item()) <= 1e-5


# ================================================================================================ 6. executors
def _episode_batch(V, D, special, seed=4):
    tok, mask, last, every = ref.episode(V, special)
    return dict(input_ids=tok, attention_mask=mask, labels=every, clip_embeddings=torch.randn(3, 3, D, generator=torch.Generator().manual_seed(seed)))


def test_clipcap_executor_trains_on_episode_batches():
    from test_executor_gpu import make_executor, vqa_batch
    z = load_golden(FIXTURES[("gpt2", "mlp")])
    ex, tok, (V, E, NLAY, NH, L, D) = make_executor(z, torch.float32)
    special = V - 5
    ex.config.data_loader.additional.special_token_id = special
    ex.config.data_loader.additional.num_shots = 2
    batch = _episode_batch(V, D, special)
    ex.model.train()
    got = ex.training_step(batch, 0)["loss"]
    want = ex.model.forward_fewshot(batch["input_ids"], batch["clip_embeddings"], batch["attention_mask"], batch["labels"], num_shots=2,
                                    special_token_id=special).loss
    assert torch.equal(got, want)
    with pytest.raises(KeyError, match="labels"):
        ex.training_step({k: v for k, v in batch.items() if k != "labels"}, 0)
    # [B, n_img, 1, D] embeddings are the same episode; one image per row still takes the <BOS> rule
    assert torch.equal(ex.training_step(dict(batch, clip_embeddings=batch["clip_embeddings"][:, :, None]), 0)["loss"], want)
    one = vqa_batch(V, D, tok.bos_token_id, tok.eos_token_id, 100)
    assert torch.isfinite(ex.training_step(one, 0)["loss"]).item()
    ex.config.data_loader.additional.num_shots = 3
    with pytest.raises(ValueError, match="num_shots"):
        ex.training_step(batch, 0)
    ex.config.data_loader.additional.num_shots = 2
    before = {k: v.clone() for k, v in ex.model.clip_project.state_dict().items()}
    losses = ex.fit([batch, batch], accumulate_grad_batches=1)
    assert ex.global_step == 2 and all(torch.isfinite(l).item() for l in losses)
    after = ex.model.clip_project.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert any(not torch.equal(before[k], after[k]) for k in before)


def test_vct0_executors_train_on_prompts_under_the_new_key():
    from test_t5_gpu import _model
    from eavqa_amd.trainers.vct0_executor import FewShotVQAExecutor, VCT0Executor
    from eavqa_amd.utils import config_system as cs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z, T_, model, V = _model("t0", torch.float32)
    D = int(z["cfg"][7])
    special = V - 1
    tok, mask, _, _ = ref.episode(V, special)
    labels = T_(z["labels"])
    episode = dict(input_ids=tok, attention_mask=mask, labels=labels, clip_embeddings=torch.randn(3, 3, D, generator=torch.Generator().manual_seed(8)))
    caption = dict(input_ids=tok, attention_mask=mask, labels=labels, clip_embeddings=T_(z["prefix"]))
    cfg = cs.load_config(os.path.join(root, "configs", "conceptual_captions", "vct0_t0_3b.jsonnet"))
    few = cs.load_config(os.path.join(root, "configs", "vqa2", "few_shot_vqa_t0_3b.jsonnet"), mode="test",
                         opts=[f"data_loader.additional.special_token_id={special}"])
    ex = VCT0Executor(cfg, model=model, dtype=torch.float32, device=DEV)
    fx = FewShotVQAExecutor(few, model=model, dtype=torch.float32, device=DEV)
    # without the key: the caption step, whatever else the batch holds; the few-shot executor does not train
    assert torch.equal(ex.training_step(caption, 0)["loss"], model(prefix=caption["clip_embeddings"], labels=labels).loss)
    assert fx.training_step(episode, 0) is None
    # with it
    cfg.data_loader.additional.train_on_prompts = True
    cfg.data_loader.additional.special_token_id = special
    few.data_loader.additional.train_on_prompts = True
    want = model(prefix=episode["clip_embeddings"], labels=labels, question_tokens=tok, question_mask=mask, special_token_id=special).loss
    assert not torch.equal(want, model(prefix=caption["clip_embeddings"], labels=labels).loss)
    assert torch.equal(ex.training_step(episode, 0)["loss"], want)
    assert torch.equal(fx.training_step(episode, 0)["loss"], want)
    assert ex._generative_step(episode, 6) is None and torch.equal(ex.logged["test/loss"], want)      # the test loss reads the prompt too
    before = {k: v.clone() for k, v in model.clip_project.state_dict().items()}
    losses = ex.fit([episode, episode], accumulate_grad_batches=1)
    after = model.clip_project.state_dict()
    assert ex.global_step == 2 and all(torch.isfinite(l).item() for l in losses)
    assert all(bool(torch.isfinite(v).all()) for v in after.values()) and any(not torch.equal(before[k], after[k]) for k in before)
