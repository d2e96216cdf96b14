"""GPU: the host-side mirror of the reference model classes (eavqa_amd.models) through the C ABI,
against the golden fixtures generated from the reference and against the oracle.

float32 mode must reproduce the reference's fp32 CPU logits/loss/grads to <= 1e-3 (north_star; we
assert 2e-4 on the tiny models) and its generated ids exactly.  bfloat16 mode (bf16 operands, fp32
accumulation and fp32 residual stream) is held to a stated looser tolerance.
"""
import math
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle
from conftest import load_golden

DEV = "cuda"
TOL = {torch.float32: dict(logits=2e-4, loss=2e-5, grad=2e-4), torch.bfloat16: dict(logits=6e-2, loss=2e-2, grad=5e-2)}


def T(a):
    return torch.from_numpy(np.asarray(a))


def sub(z, prefix):
    return {k[len(prefix):]: T(v) for k, v in z.items() if k.startswith(prefix)}


def build_model(z, arch, mapping_type, dtype):
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig
    if arch == "gpt2":
        V, E, NLAY, NH, NPOS, L, D, CL, NL = [int(v) for v in z["cfg"]]
        cfg = LMConfig("gpt2", NLAY, NH, E, 4 * E, V, NPOS, 1e-5, "gelu_new", V - 1, None)
    else:
        V, E, NLAY, NH, NPOS, L, D, FFN = [int(v) for v in z["cfg"]]
        CL, NL = None, 8
        cfg = LMConfig("opt", NLAY, NH, E, FFN, V, NPOS, 1e-5, "relu", 2, 1)
    lm = FrozenCausalLM(cfg, sub(z, "lm."), dtype, DEV)
    model = ClipCaptionPrefix(prefix_length=L, clip_length=CL, prefix_size=D, num_layers=NL, mapping_type=mapping_type,
                              lm=lm, dtype=dtype, device=DEV)
    missing = model.clip_project.load_state_dict(sub(z, "map."), strict=True)
    return model


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("arch,mapping_type,fixture", [
    ("gpt2", "mlp", "clipcap_gpt2_mlp.npz"),
    ("gpt2", "transformer", "clipcap_gpt2_transformer.npz"),
    ("opt", "mlp", "clipcap_opt_mlp.npz"),
])
@pytest.mark.parametrize("pack", [False, True])
def test_forward_loss_logits_and_mapper_grads_match_reference(dtype, arch, mapping_type, fixture, pack):
    """pack=True is the default training path (padded positions dropped before the first GEMM): loss, gradients and
    the logits of every attended position must still match the reference; pack=False also matches the (unused)
    logits the reference computes at padded positions."""
    z = load_golden(fixture)
    model = build_model(z, arch, mapping_type, dtype).train()
    model.pack_padding = pack
    out = model(question_tokens=T(z["ids"]), prefix=T(z["prefix"]), question_mask=T(z["mask"]), labels=T(z["labels"]),
                pad_token_id=int(z["pad_id"]))
    tol = TOL[dtype]
    assert out.logits.shape == z["logits"].shape
    diff = (out.logits.float().cpu() - T(z["logits"])).abs()
    if pack:
        L = z["logits"].shape[1] - z["mask"].shape[1]
        attended = torch.cat([torch.ones(z["mask"].shape[0], L, dtype=torch.bool), T(z["mask"]) != 0], dim=1)
        assert (out.logits.float().cpu()[~attended] == 0).all()
        diff = diff[attended]
    assert diff.max().item() <= tol["logits"]
    assert abs(out.loss.item() - float(z["loss"])) <= tol["loss"]
    out.loss.backward()
    for k, g in sub(z, "g.").items():
        p = dict(model.clip_project.named_parameters())[k]
        assert p.grad is not None, k
        err = (p.grad.cpu() - g).abs().max().item()
        assert err <= tol["grad"] * max(1.0, g.abs().max().item()), (k, err)


def test_backward_accumulates_and_zero_grad_resets():
    z = load_golden("clipcap_gpt2_mlp.npz")
    model = build_model(z, "gpt2", "mlp", torch.float32).train()
    args = dict(question_tokens=T(z["ids"]), prefix=T(z["prefix"]), question_mask=T(z["mask"]), labels=T(z["labels"]))
    model(**args).loss.backward()
    g1 = {k: p.grad.clone() for k, p in model.clip_project.named_parameters()}
    model(**args).loss.backward()                      # accumulate_grad_batches semantics (src/main.py:118)
    for k, p in model.clip_project.named_parameters():
        assert torch.allclose(p.grad, 2 * g1[k], atol=1e-6, rtol=1e-5), k
    model.clip_project.zero_grad(set_to_none=True)
    model(**args).loss.backward()
    for k, p in model.clip_project.named_parameters():
        assert torch.allclose(p.grad, g1[k], atol=1e-6, rtol=1e-5), k


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("mapping_type", ["mlp", "transformer"])
def test_generate_ids_exact_fp32(mapping_type, use_cache):
    z = load_golden(f"clipcap_gpt2_{mapping_type}.npz")
    model = build_model(z, "gpt2", mapping_type, torch.float32).eval()
    pad = int(z["pad_id"])
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=6,
              pad_token_id=pad, use_cache=use_cache)
    assert model.generate(eos_token_id=None, **kw) == z["gen_free"].tolist()
    assert model.generate(eos_token_id=int(z["gen_forced_eos"]), **kw) == z["gen_forced"].tolist()
    early = model.generate(question_tokens=T(z["gen_ids"])[:1], prefix=T(z["prefix"])[:1], question_mask=T(z["gen_mask"])[:1],
                           max_length=6, pad_token_id=pad, eos_token_id=int(z["gen_early_eos"]), use_cache=use_cache)
    assert early == z["gen_early"].tolist()


@pytest.mark.parametrize("use_cache", [True, False])
def test_generate_scores_match_oracle_fp32(use_cache):
    """``output_scores=True``: per-token log-probabilities (what the few-shot ensembling sums,
    few_shot_vqa_executor.py:314-322) against the oracle's log_softmax at the greedy token."""
    from oracle import ref_cpu
    z = load_golden("clipcap_gpt2_mlp.npz")
    model = build_model(z, "gpt2", "mlp", torch.float32).eval()
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=6,
              pad_token_id=int(z["pad_id"]), eos_token_id=None)
    ids, lp = model.generate(use_cache=use_cache, output_scores=True, **kw)
    assert ids == z["gen_free"].tolist() and tuple(lp.shape) == (len(ids), len(ids[0]))
    V, E, NLAY, NH, NPOS, L, D, CL, NL = [int(v) for v in z["cfg"]]
    with torch.no_grad():
        oids, olp = ref_cpu.clipcap_generate(sub(z, "lm."), dict(arch="gpt2", n_layer=NLAY, n_head=NH), sub(z, "map."),
                                             dict(prefix_length=L, clip_length=CL, num_layers=NL, mapping_type="mlp"), T(z["gen_ids"]),
                                             T(z["prefix"]), T(z["gen_mask"]), max_length=6, pad_token_id=int(z["pad_id"]),
                                             eos_token_id=None, output_scores=True)
    assert oids == ids
    assert (lp - olp).abs().max().item() <= 1e-4


@pytest.mark.parametrize("use_cache", [True, False])
def test_generate_opt_ids_exact_fp32(use_cache):
    z = load_golden("clipcap_opt_mlp.npz")
    model = build_model(z, "opt", "mlp", torch.float32).eval()
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=5,
              pad_token_id=int(z["pad_id"]), use_cache=use_cache)
    assert model.generate(eos_token_id=None, **kw) == z["gen_free"].tolist()
    assert model.generate(eos_token_id=int(z["gen_forced_eos"]), **kw) == z["gen_forced"].tolist()


def test_generate_requires_pad_when_eos_given():
    z = load_golden("clipcap_gpt2_mlp.npz")
    model = build_model(z, "gpt2", "mlp", torch.float32).eval()
    with pytest.raises(ValueError, match="pad_token_id"):   # clipcap.py:426-430
        model.generate(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]),
                       max_length=2, pad_token_id=None, eos_token_id=5)


def test_bf16_cached_and_uncached_generation_agree():
    z = load_golden("clipcap_gpt2_mlp.npz")
    model = build_model(z, "gpt2", "mlp", torch.bfloat16).eval()
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=6,
              pad_token_id=int(z["pad_id"]), eos_token_id=None)
    a = model.generate(use_cache=True, **kw)
    b = model.generate(use_cache=False, **kw)
    agree = np.mean(np.array(a) == np.array(b))
    assert agree >= 0.75, (a, b)     # same math, different summation order in bf16: near-ties may flip


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["clip_vit.npz", "clip_vit_p14.npz"])
def test_clip_vit_matches_reference(dtype, name):
    from eavqa_amd.models.clip_vit import ClipVisionEncoder, ViTConfig
    z = load_golden(name)
    W, MLP, NL, NH, IMG, P, D = [int(v) for v in z["cfg"]]
    enc = ClipVisionEncoder(ViTConfig(W, NL, NH, MLP, P, IMG, D), sub(z, "w."), dtype, DEV)
    emb = enc.encode_image(T(z["pixels"]))
    assert emb.dtype == torch.float32 and emb.shape == (z["pixels"].shape[0], D)
    err = (emb.cpu() - T(z["image_embeds"])).abs().max().item()
    assert err <= (2e-4 if dtype == torch.float32 else 5e-2), err


def test_real_shape_gpt2_small_fp32_logits_within_1e3_of_oracle():
    """BASELINE config 1 shape (ViT-B/32 -> GPT-2 small, MLP mapper, B=4, S=10+32), random init, fp32 path:
    logits within 1e-3 of the CPU oracle (north_star tolerance), loss within 1e-4."""
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, KNOWN_CONFIGS, random_init_state_dict
    cfg = LMConfig.from_hf_dict(KNOWN_CONFIGS["gpt2"])
    cfg.n_layer = 4                     # 4 of 12 layers keeps the CPU oracle to a few seconds
    sd = random_init_state_dict(cfg, 2021, "cpu")
    lm = FrozenCausalLM(cfg, sd, torch.float32, DEV)
    torch.manual_seed(0)
    model = ClipCaptionPrefix(prefix_length=10, prefix_size=512, mapping_type="mlp", lm=lm, dtype=torch.float32, device=DEV).train()
    g = torch.Generator().manual_seed(2021)
    B, Tt = 4, 32
    lens = torch.randint(8, Tt + 1, (B,), generator=g); lens[0] = Tt
    ids = torch.randint(0, 50255, (B, Tt), generator=g)
    mask = (torch.arange(Tt)[None] < lens[:, None]).long()
    ids = ids * mask + 50256 * (1 - mask)
    labels = oracle.label_mask_cc(ids, 50256)
    prefix = torch.randn(B, 512, generator=g)
    model.pack_padding = False
    out = model(question_tokens=ids, prefix=prefix, question_mask=mask, labels=labels)
    mapper = {k: v.detach().cpu() for k, v in model.clip_project.state_dict().items()}
    ocfg = dict(arch="gpt2", n_layer=cfg.n_layer, n_head=cfg.n_head)
    loss, logits = oracle.clipcap_forward(sd, ocfg, mapper, dict(prefix_length=10, mapping_type="mlp"), ids, prefix, mask, labels)
    assert (out.logits.cpu() - logits).abs().max().item() <= 1e-3
    assert abs(out.loss.item() - loss.item()) <= 1e-4


def test_packed_and_padded_training_steps_agree_fp32():
    """Dropping the padded rows changes neither the loss nor the mapper gradients (beyond fp32 summation order),
    with the lengths given by the host or read back from the device."""
    z = load_golden("clipcap_gpt2_mlp.npz")
    model = build_model(z, "gpt2", "mlp", torch.float32).train()
    args = dict(question_tokens=T(z["ids"]), prefix=T(z["prefix"]), question_mask=T(z["mask"]), labels=T(z["labels"]))
    res = {}
    n_lab = int((T(z["labels"]) != -100).sum())
    for name, pack, kw in (("padded", False, {}), ("packed_host_lengths", True, {}),
                           ("packed_device_lengths", True, dict(question_mask=T(z["mask"]).to(DEV))),
                           ("packed_all_rows_scored", True, dict(labels=T(z["labels"]).to(DEV))),          # device labels: no count
                           ("packed_count_hint", True, dict(labels=T(z["labels"]).to(DEV), label_count=n_lab)),
                           ("packed_count_overestimate", True, dict(labels=T(z["labels"]).to(DEV), label_count=n_lab + 3))):
        model.pack_padding = pack
        model.clip_project.zero_grad(set_to_none=True)
        out = model(**{**args, **kw})
        out.loss.backward()
        res[name] = (out.loss.item(), {k: p.grad.clone() for k, p in model.clip_project.named_parameters()})
    for name in ("packed_host_lengths", "packed_device_lengths", "packed_all_rows_scored", "packed_count_hint", "packed_count_overestimate"):
        assert abs(res[name][0] - res["padded"][0]) <= 1e-6
        for k, g in res["padded"][1].items():
            assert torch.allclose(res[name][1][k], g, atol=1e-6, rtol=1e-5), (name, k)
    # .logits after a scored-rows-only forward is computed on demand and equals the all-rows packed result
    model.pack_padding = True
    a = model(**{**args, "labels": T(z["labels"]).to(DEV)}).logits.cpu()             # every packed row through the head
    b = model(**{**args, "label_count": n_lab}).logits.cpu()
    assert torch.equal(a, b)


def _oracle_fewshot_generate(sd, cfg, mapper, L, tokens, prefix, mask, n_img, special, max_length, pad, eos):
    """Few-shot greedy decode restated with the oracle: mapper on every image, insert_prefix_into_input
    (vct0.py:494-533), then the clipcap greedy loop (clipcap.py:387-471) on the joint embeddings."""
    wte = sd["transformer.wte.weight"] if cfg["arch"] == "gpt2" else sd["model.decoder.embed_tokens.weight"]
    B = tokens.shape[0]
    E = wte.shape[1]
    pp = oracle.mlp_mapper(prefix.reshape(B * n_img, -1), mapper).reshape(B, n_img, L, E)
    emb, am = oracle.insert_prefix_into_input(L, n_img - 1, tokens, wte[tokens], pp, mask, special_token_id=special)
    am = am.float()
    unfinished = torch.ones(B, 1)
    toks = None
    for _ in range(max_length):
        logits = oracle.lm_logits(sd, cfg, emb, am)
        nxt = torch.argmax(logits[:, -1, :], -1).unsqueeze(1)
        emb = torch.cat((emb, wte[nxt]), dim=1)
        if eos is not None:
            nxt = nxt * unfinished + pad * (1 - unfinished)
        toks = nxt if toks is None else torch.cat((toks, nxt), dim=1)
        am = torch.cat([am, torch.ones(B, 1)], dim=-1)
        if eos is not None:
            unfinished = unfinished.mul((nxt != eos).long())
        if unfinished.max() == 0:
            break
    return toks.numpy().astype(int).tolist()


@pytest.mark.parametrize("arch,fixture", [("gpt2", "clipcap_gpt2_mlp.npz"), ("opt", "clipcap_opt_mlp.npz")])
@pytest.mark.parametrize("use_cache", [True, False])
def test_fewshot_generate_matches_oracle_fp32(arch, fixture, use_cache):
    """4-shot-style prompt (3 images per row here): sentinel tokens expand into the mapper's prefix rows and the
    greedy ids equal the oracle's (insert_prefix_into_input + reference greedy loop), float32, exact."""
    z = load_golden(fixture)
    model = build_model(z, arch, "mlp", torch.float32).eval()
    V = int(z["cfg"][0]); D = int(z["cfg"][6]); L = model.prefix_length
    g = torch.Generator().manual_seed(9)
    B, n_img, seg = 3, 3, 4
    special = V - 5
    T_ = n_img * (1 + seg) + 2
    tok = torch.randint(3, special - n_img - 1, (B, T_), generator=g)
    for b in range(B):
        for i in range(n_img):
            tok[b, i * (1 + seg) + (b % 2)] = special - i       # sentinel positions differ between rows
    mask = torch.ones(B, T_, dtype=torch.long)
    mask[1, -2:] = 0                                              # right padding on one row
    prefix = torch.randn(B, n_img, D, generator=g)
    pad = int(z["pad_id"])
    sd, mapper = sub(z, "lm."), sub(z, "map.")
    cfg = dict(arch=arch, n_layer=int(z["cfg"][2]), n_head=int(z["cfg"][3]))
    with torch.no_grad():
        want = _oracle_fewshot_generate(sd, cfg, mapper, L, tok, prefix, mask, n_img, special, 5, pad, None)
    got = model.generate_fewshot(tok, prefix, mask, num_shots=n_img - 1, special_token_id=special, max_length=5,
                                 pad_token_id=pad, eos_token_id=None, use_cache=use_cache)
    assert got == want
    # ensembling over two "permutations" of the in-context images: per-token log-probs feed the sequence scores
    # (few_shot_vqa_executor.py:293-332); permuting the first two images changes the prompt, the selection is per question
    from eavqa_amd.utils import ensembling
    perms = [prefix, prefix[:, [1, 0, 2]]]
    runs = [model.generate_fewshot(tok, p_, mask, num_shots=n_img - 1, special_token_id=special, max_length=5, pad_token_id=pad,
                                   eos_token_id=None, use_cache=use_cache, output_scores=True) for p_ in perms]
    assert runs[0][0] == want and tuple(runs[0][1].shape) == (B, 5) and bool((runs[0][1] <= 0).all())
    best = ensembling.generate_from_ensembles(lambda i: runs[i], 2)
    sc = np.stack([ensembling.sequence_scores(r[0], r[1]) for r in runs], 1)
    assert best == [runs[int(np.argmax(sc[j]))][0][j] for j in range(B)]
    bad = tok.clone(); bad[0, 0] = 3; bad[0, 1] = 4     # row 0 loses a sentinel (it sat at index 0)
    if (bad[0] > special - n_img).sum() != n_img:
        with pytest.raises(ValueError, match="sentinel"):
            model.generate_fewshot(bad, prefix, mask, num_shots=n_img - 1, special_token_id=special, max_length=2,
                                   pad_token_id=pad, eos_token_id=None)


def _tiny_lm(V=96, E=64, n_layer=2, n_head=4, n_pos=400, seed=3, arch="gpt2"):
    from eavqa_amd.models.lm import LMConfig, random_init_state_dict
    cfg = LMConfig(arch, n_layer, n_head, E, 4 * E if arch == "gpt2" else 96, V, n_pos, 1e-5, "gelu_new" if arch == "gpt2" else "relu",
                   V - 1, None if arch == "gpt2" else 1)
    sd = random_init_state_dict(cfg, seed, "cpu")
    for k in sd:                      # HF init leaves biases at 0 and LayerNorm at 1/0: perturb so they are exercised
        if k.endswith("bias") or "ln_" in k or "layer_norm" in k:
            g = torch.Generator().manual_seed(zlib.crc32(k.encode()) % 1000)      # (str hash() differs from process to process)
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
    return cfg, sd


@pytest.mark.parametrize("arch", ["gpt2", "opt"])
@pytest.mark.parametrize("B,Tt,lens", [
    (1, 1, [1]),                 # a single token
    (3, 1, [1, 1, 1]),
    (2, 300, [300, 17]),         # several attention tiles, one row mostly padding
    (5, 33, [33, 1, 2, 32, 16]), # ragged, odd batch
    (2, 8, [8, 0]),              # a row with NO attended text token (only the prefix is attended)
])
def test_edge_shapes_match_oracle_fp32(arch, B, Tt, lens):
    """Ragged / degenerate batches through the packed training forward: loss, attended logits and mapper gradients
    against the oracle (float32)."""
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM
    cfg, sd = _tiny_lm(arch=arch)
    L, D = 3, 16
    lm = FrozenCausalLM(cfg, sd, torch.float32, DEV)
    torch.manual_seed(1)
    model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=torch.float32, device=DEV).train()
    g = torch.Generator().manual_seed(B * 1000 + Tt)
    pad = cfg.vocab - 1
    ids = torch.randint(2, cfg.vocab - 2, (B, Tt), generator=g)
    mask = (torch.arange(Tt)[None] < torch.tensor(lens)[:, None]).long()
    ids = ids * mask + pad * (1 - mask)
    labels = oracle.label_mask_cc(ids, pad)
    prefix = torch.randn(B, D, generator=g)
    out = model(question_tokens=ids, prefix=prefix, question_mask=mask, labels=labels)
    mapper = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.clip_project.state_dict().items()}
    ocfg = dict(arch=arch, n_layer=cfg.n_layer, n_head=cfg.n_head, act=cfg.act)
    loss, logits = oracle.clipcap_forward(sd, ocfg, mapper, dict(prefix_length=L, mapping_type="mlp"), ids, prefix, mask, labels)
    attended = torch.cat([torch.ones(B, L, dtype=torch.bool), mask.bool()], dim=1)
    assert (out.logits.cpu()[attended] - logits.detach()[attended]).abs().max().item() <= 2e-4
    if torch.isnan(loss):                       # no labelled position at all: mean over nothing, as torch
        assert torch.isnan(out.loss).item()
        return
    assert abs(out.loss.item() - loss.item()) <= 5e-5
    out.loss.backward()
    loss.backward()
    for k, p in model.clip_project.named_parameters():
        want = mapper[k].grad
        assert (p.grad.cpu() - want).abs().max().item() <= 2e-4 * max(1.0, want.abs().max().item()), k


def test_full_size_cfg2_properties_bf16():
    """BASELINE configs[1] at its real size (GPT-2-large, 36 layers, E = 1280, MLP mapper 512 -> 6400 -> 12800, bf16; batch 16
    of the 64 to keep the test short) through size-independent properties, since the CPU oracle cannot run it in seconds:
    the packed and the padded training step agree on loss and mapper gradients, two identical steps are bitwise equal,
    the gradient is linear in the upstream scale, and cached / uncached greedy decoding agree on the first token."""
    from eavqa_amd.data.synthetic import cc_batch
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, KNOWN_CONFIGS, random_init_state_dict
    cfg = LMConfig.from_hf_dict(KNOWN_CONFIGS["gpt2-large"])
    lm = FrozenCausalLM(cfg, random_init_state_dict(cfg, 2021, DEV), torch.bfloat16, DEV)
    torch.manual_seed(2021)
    model = ClipCaptionPrefix(prefix_length=10, prefix_size=512, mapping_type="mlp", lm=lm, dtype=torch.bfloat16, device=DEV).train()
    b = cc_batch(16, cfg.vocab, cfg.eos_token_id, max_len=32, seed=7, device=DEV, with_pixels=False, embed_dim=512)
    kw = dict(question_tokens=b["input_ids"], prefix=b["clip_embeddings"], question_mask=b["attention_mask"], labels=b["labels"],
              pad_token_id=cfg.eos_token_id)

    def step(pack, scale=1.0):
        model.pack_padding = pack
        model.clip_project.zero_grad(set_to_none=True)
        out = model(**kw)
        (out.loss * scale).backward()
        return out.loss.item(), {k: p.grad.clone() for k, p in model.clip_project.named_parameters()}

    l_pack, g_pack = step(True)
    l_pad, g_pad = step(False)
    assert math.isfinite(l_pack) and abs(l_pack - l_pad) <= 2e-2 * abs(l_pad)
    for k in g_pad:
        den = g_pad[k].abs().max().item()
        assert (g_pack[k] - g_pad[k]).abs().max().item() <= 5e-2 * den, k
    l2, g2 = step(True)
    assert l2 == l_pack and all(torch.equal(g2[k], g_pack[k]) for k in g2)          # fixed-order reductions everywhere
    _, g3 = step(True, scale=4.0)
    for k in g3:
        assert (g3[k] - 4.0 * g_pack[k]).abs().max().item() <= 2e-2 * 4.0 * g_pack[k].abs().max().item(), k
    model.eval()
    gen = dict(question_tokens=b["input_ids"][:4, :8], prefix=b["clip_embeddings"][:4], question_mask=b["attention_mask"][:4, :8],
               max_length=1, pad_token_id=cfg.eos_token_id, eos_token_id=None)
    assert model.generate(use_cache=True, **gen) == model.generate(use_cache=False, **gen)


@pytest.mark.parametrize("arch,B", [("gpt2", 5), ("opt", 33), ("opt", 64)])
def test_decode_fast_path_logits_match_full_forward_bf16(arch, B):
    """The bf16 decode step (C driver: split-K GEMMs + fused finish / LayerNorm + decode attention over the KV cache) against
    the logits of a full re-forward over the grown sequence - the reference's own algorithm (clipcap.py:414-419) - for three
    consecutive steps, with ragged prompt masks.  Same bf16 operands, different summation orders."""
    from eavqa_amd import ops
    from eavqa_amd.models import decode as dec
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, random_init_state_dict
    E, H, F, NL, V, NPOS = 256, 4, 1024, 2, 512, 64
    cfg = (LMConfig("gpt2", NL, H, E, F, V, NPOS, 1e-5, "gelu_new", V - 1, None) if arch == "gpt2"
           else LMConfig("opt", NL, H, E, F, V, NPOS, 1e-5, "relu", 2, 1))
    lm = FrozenCausalLM(cfg, random_init_state_dict(cfg, 5, DEV), torch.bfloat16, DEV)
    g = torch.Generator().manual_seed(B)
    S0, steps = 9, 3
    S_max = S0 + steps
    tok = torch.randint(3, V - 1, (B, S_max), generator=g)
    lens = torch.randint(4, S0 + 1, (B,), generator=g); lens[0] = S0
    qm = torch.ones(B, S_max, dtype=torch.long)
    qm[:, :S0] = (torch.arange(S0)[None] < lens[:, None]).long()          # right-padded prompt, generated positions attended
    src, mask, pos = ops.build_prefix_rows(tok.to(DEV), qm.to(DEV), 0, cfg.pos_mode)
    cache = dec._KVCache(lm, B, S_max, B * S0)
    logits = dec._prefill(lm, cache, None, src[:, :S0].contiguous(), pos[:, :S0].contiguous(), mask, B, S0, S_max)
    for t in range(steps + 1):
        S = S0 + t
        full = lm.forward(None, src[:, :S].contiguous(), pos[:, :S].contiguous(), mask[:, :S].contiguous(), B, S, logits="last")["logits"]
        a, b = logits[:, :V].float().cpu(), full[:, :V].float().cpu()
        assert (a - b).abs().max().item() <= 4e-2 * max(1.0, b.abs().max().item()), (t, (a - b).abs().max().item())
        if t == steps:
            break
        raw = src[:, S].contiguous()                                       # teacher-forced next token
        logits = dec._decode_step(lm, cache, raw, pos[:, S].contiguous(), mask, B, S, S_max)


@pytest.mark.parametrize("mapping_type", ["mlp", "transformer"])
def test_pipelined_adamw_is_bit_equal_and_the_forward_waits_per_layer(mapping_type):
    """``FusedAdamW.step(chunks=mapper.update_chunks())``: the update runs chunk by chunk on the optimiser's stream and the mapper's next
    forward waits for the ranges it reads (``FlatParams.wait_ready``) - same parameters, bit for bit, as the one-launch update after three
    training steps, for both mappers; the chunks partition the flat buffer in forward order."""
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, random_init_state_dict
    from eavqa_amd.trainers.optim import FusedAdamW
    cfg = LMConfig("gpt2", 2, 4, 64, 256, 320, 64, 1e-5, "gelu_new", 319, None)
    sd = random_init_state_dict(cfg, 3, "cpu")
    g = torch.Generator().manual_seed(5)
    B, T, D, L = 6, 12, 24, 4
    ids = torch.randint(3, 300, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    labels = ids.clone()
    prefix = torch.randn(B, D, generator=g)
    finals = []
    for pipelined in (False, True):
        lm = FrozenCausalLM(cfg, sd, torch.bfloat16, DEV)
        torch.manual_seed(1)
        model = ClipCaptionPrefix(prefix_length=L, clip_length=L, prefix_size=D, num_layers=3, mapping_type=mapping_type, lm=lm, dtype=torch.bfloat16,
                                  device=DEV).train()
        fl = model.clip_project.flat
        chunks = model.clip_project.update_chunks()
        assert sorted(chunks)[0][0] == 0 and sum(h - l for l, h in chunks) == fl.numel and chunks[0] == (0, fl.small_numel)
        spans = sorted(chunks)
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))          # a partition: no gap, no overlap
        opt = FusedAdamW(fl, lr=1e-2)
        for _ in range(3):
            out = model(question_tokens=ids, prefix=prefix, question_mask=mask, labels=labels)
            out.loss.backward()
            opt.step(chunks=chunks if pipelined else None)
            opt.zero_grad()
            if pipelined:
                assert fl._ready                                            # the update is pending until a forward (or wait_ready) takes it
        fl.wait_ready()
        torch.cuda.synchronize()
        finals.append((fl.master.clone(), fl.shadow.clone(), float(out.loss.item())))
    assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1]) and finals[0][2] == finals[1][2]


@pytest.mark.parametrize("arch", ["gpt2", "opt"])
@pytest.mark.parametrize("pack", [False, True])
def test_folded_layernorm_training_step_matches_the_layernorm_kernels_bf16(arch, pack):
    """``FrozenCausalLM.fold_layernorm`` (eavqa_gemm_ln: ln_1 / ln_2 as an epilogue term of the QKV / FFN-up products, the stream's row
    sums and bf16 copy written by the out-projection / FFN-down epilogues) against the same bf16 model with the LayerNorm kernels, and
    both against the fp32 oracle: the folded step must sit as close to the oracle as the unfolded one (the two differ from each other by
    bf16 roundings taken at different places: of x instead of LayerNorm(x), of W gamma instead of W)."""
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM
    cfg, sd = _tiny_lm(V=320, E=128, n_layer=4, n_head=4, arch=arch)
    L, D, B, Tt = 4, 24, 9, 20                                     # 216 rows padded, ~170 packed: above the 64-row limit of the fold
    g = torch.Generator().manual_seed(11)
    pad = cfg.vocab - 1
    lens = torch.randint(8, Tt + 1, (B,), generator=g)
    ids = torch.randint(2, cfg.vocab - 2, (B, Tt), generator=g)
    mask = (torch.arange(Tt)[None] < lens[:, None]).long()
    ids = ids * mask + pad * (1 - mask)
    labels = oracle.label_mask_cc(ids, pad)
    prefix = torch.randn(B, D, generator=g)
    res = {}
    for fold in (False, True):
        lm = FrozenCausalLM(cfg, sd, torch.bfloat16, DEV)
        assert not lm.fold_layernorm                               # an option (EAVQA_LN_FOLD=1), measured equal: off by default
        lm.fold_layernorm = fold
        torch.manual_seed(1)
        model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=torch.bfloat16, device=DEV).train()
        model.pack_padding = pack
        out = model(question_tokens=ids, prefix=prefix, question_mask=mask, labels=labels)
        out.loss.backward()
        torch.cuda.synchronize()
        res[fold] = (out.loss.item(), out.logits.float().cpu(), {k: p.grad.float().cpu().clone() for k, p in model.clip_project.named_parameters()})
        mapper = {k: v.detach().float().cpu().clone().requires_grad_(True) for k, v in model.clip_project.state_dict().items()}
    ocfg = dict(arch=arch, n_layer=cfg.n_layer, n_head=cfg.n_head, act=cfg.act)
    loss, logits = oracle.clipcap_forward(sd, ocfg, mapper, dict(prefix_length=L, mapping_type="mlp"), ids, prefix, mask, labels)
    loss.backward()
    attended = torch.cat([torch.ones(B, L, dtype=torch.bool), mask.bool()], dim=1)
    err = {f: (res[f][1][attended] - logits.detach()[attended]).abs().max().item() for f in res}
    assert err[True] <= max(1.5 * err[False], 2e-2), err
    assert abs(res[True][0] - loss.item()) <= max(1.5 * abs(res[False][0] - loss.item()), 3e-3)
    for k in res[True][2]:
        want = mapper[k].grad
        e = {f: (res[f][2][k] - want).abs().max().item() for f in res}
        assert e[True] <= max(1.5 * e[False], 2e-2 * want.abs().max().item()), (k, e)


def test_encode_ahead_returns_the_embeddings_and_ids_of_the_sequential_loop():
    """``EncodeAhead`` (the image tower of batch i + 1 on a second stream while batch i is generated): embeddings bit-equal with
    ``encode_image`` on the calling stream, generated ids equal over three pipelined batches with different images."""
    from eavqa_amd.models.clip_vit import ClipVisionEncoder, EncodeAhead, ViTConfig, random_init_vit_state_dict
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM
    vcfg = ViTConfig(64, 2, 2, 128, 8, 32, 24)                     # width, layers, heads, mlp, patch, image, projection
    vit = ClipVisionEncoder(vcfg, random_init_vit_state_dict(vcfg, 5, DEV), torch.bfloat16, DEV)
    cfg, sd = _tiny_lm(V=160, E=64, n_layer=2, n_head=4)
    lm = FrozenCausalLM(cfg, sd, torch.bfloat16, DEV)
    torch.manual_seed(1)
    model = ClipCaptionPrefix(prefix_length=3, prefix_size=24, mapping_type="mlp", lm=lm, dtype=torch.bfloat16, device=DEV).eval()
    g = torch.Generator().manual_seed(4)
    B, T, n = 5, 7, 3
    px = [torch.randn(B, 3, 32, 32, generator=g).to(DEV) for _ in range(n)]
    ids = torch.randint(3, 150, (B, T), generator=g).to(DEV)
    mask = torch.ones(B, T, dtype=torch.long, device=DEV)
    gen = lambda emb: model.generate(question_tokens=ids, prefix=emb, question_mask=mask, max_length=6, pad_token_id=0)
    want_emb = [vit.encode_image(p) for p in px]
    want = [gen(e) for e in want_emb]
    ahead = EncodeAhead(vit)
    ticket = ahead.submit(px[0])
    for i in range(n):
        emb = ahead.result(ticket)
        if i + 1 < n:
            ticket = ahead.submit(px[i + 1])
        got = gen(emb)
        torch.cuda.synchronize()
        assert torch.equal(emb, want_emb[i]) and got == want[i], i
