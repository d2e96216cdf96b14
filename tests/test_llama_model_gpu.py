"""GPU: the Llama family behind ClipCaptionPrefix against tests/golden/clipcap_llama_mlp.npz - the REFERENCE's own forward / generate
code driving a tiny HF ``LlamaForCausalLM`` (4 heads over 2 key / value heads; tests/golden/make_golden_llama.py) - at the tolerances
of tests/test_model_gpu.py, and the cached generation route against the re-forward route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden

DEV = "cuda"
TOL = {torch.float32: dict(logits=2e-4, loss=2e-5, grad=2e-4), torch.bfloat16: dict(logits=6e-2, loss=2e-2, grad=5e-2)}
FIXTURE = "clipcap_llama_mlp.npz"


def T(a):
    return torch.from_numpy(np.asarray(a))


def sub(z, prefix):
    return {k[len(prefix):]: T(v) for k, v in z.items() if k.startswith(prefix)}


def llama_config(z):
    from eavqa_amd.models.lm import LMConfig
    V, E, NLAY, NH, NPOS, L, D, FFN, NKV = [int(v) for v in z["cfg"]]
    cfg = LMConfig.from_hf_dict(dict(model_type="llama", vocab_size=V, hidden_size=E, num_hidden_layers=NLAY, num_attention_heads=NH,
                                     num_key_value_heads=NKV, intermediate_size=FFN, max_position_embeddings=NPOS,
                                     rms_norm_eps=float(z["rms_norm_eps"]), rope_theta=float(z["rope_theta"]), eos_token_id=2, pad_token_id=0))
    return cfg, L, D


def build_model(z, dtype):
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM
    cfg, L, D = llama_config(z)
    lm = FrozenCausalLM(cfg, sub(z, "lm."), dtype, DEV)
    model = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=DEV)
    model.clip_project.load_state_dict(sub(z, "map."), strict=True)
    return model


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pack", [False, True])
def test_forward_loss_logits_and_mapper_grads_match_reference(dtype, pack):
    z = load_golden(FIXTURE)
    model = build_model(z, dtype).train()
    model.pack_padding = pack
    out = model(question_tokens=T(z["ids"]), prefix=T(z["prefix"]), question_mask=T(z["mask"]), labels=T(z["labels"]),
                pad_token_id=int(z["pad_id"]))
    tol = TOL[dtype]
    assert out.logits.shape == z["logits"].shape
    diff = (out.logits.float().cpu() - T(z["logits"])).abs()
    L = z["logits"].shape[1] - z["mask"].shape[1]
    attended = torch.cat([torch.ones(z["mask"].shape[0], L, dtype=torch.bool), T(z["mask"]) != 0], dim=1)
    if pack:
        assert (out.logits.float().cpu()[~attended] == 0).all()
        diff = diff[attended]
    print(f"[{dtype} pack={pack}] max |d logits| {diff.max().item():.3e}  |d loss| {abs(out.loss.item() - float(z['loss'])):.3e}")
    assert diff.max().item() <= tol["logits"]
    assert abs(out.loss.item() - float(z["loss"])) <= tol["loss"]
    out.loss.backward()
    for k, g in sub(z, "g.").items():
        p = dict(model.clip_project.named_parameters())[k]
        assert p.grad is not None, k
        err = (p.grad.cpu() - g).abs().max().item()
        print(f"    grad {k}: max err {err:.3e} of {g.abs().max().item():.3e}")
        assert err <= tol["grad"] * max(1.0, g.abs().max().item()), (k, err)


@pytest.mark.parametrize("use_cache", [True, False])
def test_generate_ids_exact_fp32(use_cache):
    z = load_golden(FIXTURE)
    model = build_model(z, torch.float32).eval()
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=5,
              pad_token_id=int(z["pad_id"]), use_cache=use_cache)
    assert model.generate(eos_token_id=None, **kw) == z["gen_free"].tolist()
    assert model.generate(eos_token_id=int(z["gen_forced_eos"]), **kw) == z["gen_forced"].tolist()


def _cached_steps_against_reforward(lm, B, S0, steps, V, seed):
    """Prefill + ``steps`` teacher-forced cached steps against ``lm.forward`` over the grown sequence, ragged right-padded prompts:
    the largest logit difference of every step."""
    from eavqa_amd import ops
    from eavqa_amd.models import decode as dec
    g = torch.Generator().manual_seed(seed)
    S_max = S0 + steps
    tok = torch.randint(3, V - 1, (B, S_max), generator=g)
    lens = torch.randint(4, S0 + 1, (B,), generator=g)
    lens[0] = S0
    qm = torch.ones(B, S_max, dtype=torch.long)
    qm[:, :S0] = (torch.arange(S0)[None] < lens[:, None]).long()
    src, mask, pos = ops.build_prefix_rows(tok.to(DEV), qm.to(DEV), 0, lm.cfg.pos_mode)
    cache = dec._KVCache(lm, B, S_max, B * S0)
    logits = dec._prefill(lm, cache, None, src[:, :S0].contiguous(), pos[:, :S0].contiguous(), mask, B, S0, S_max)
    out = []
    for t in range(steps + 1):
        S = S0 + t
        full = lm.forward(None, src[:, :S].contiguous(), pos[:, :S].contiguous(), mask[:, :S].contiguous(), B, S, logits="last")["logits"]
        out.append((logits[:, :V].float() - full[:, :V].float()).abs().max().item())
        if t == steps:
            break
        logits = dec._decode_step(lm, cache, src[:, S].contiguous(), pos[:, S].contiguous(), mask, B, S, S_max)
    return out


@pytest.mark.parametrize("shape,B", [("fixture", 4), ("splitk", 5), ("splitk", 33), ("splitk", 64), ("no_down_plan", 33)])
def test_bf16_cached_step_logits_match_the_reforward(shape, B):
    """Every cached step's logits within the bf16 logits tolerance (6e-2) of the re-forward logits: the fixture's LM (whatever route its
    shapes plan), a 256-wide LM whose step takes the split-K route (rope_finish, attention_decode, swiglu_splitk), and one whose FFN
    width (1376 = 32 * 43) has no split plan for the down-projection at 33 rows, as Llama-2-7B's 11008 has none at 32: that product then
    runs as eavqa_gemm inside the split-K step.  4 heads over 2 key / value heads in all."""
    from eavqa_amd import _lib
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, random_init_state_dict
    if shape == "fixture":
        z = load_golden(FIXTURE)
        cfg, _, _ = llama_config(z)
        lm = FrozenCausalLM(cfg, sub(z, "lm."), torch.bfloat16, DEV)
    else:
        cfg = LMConfig.from_hf_dict(dict(model_type="llama", vocab_size=512, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                         num_key_value_heads=2, intermediate_size=704 if shape == "splitk" else 1376,
                                         max_position_embeddings=64, rms_norm_eps=1e-5))
        lm = FrozenCausalLM(cfg, random_init_state_dict(cfg, 5, DEV), torch.bfloat16, DEV)
        plan = _lib.load().eavqa_gemm_splitk_plan
        E, F = cfg.n_embd, cfg.ffn
        assert min(plan(B, 3 * E, E), plan(B, E, E), plan(B, 2 * F, E)) > 0                     # the step takes the split-K route
        assert (plan(B, E, F) > 0) == (shape == "splitk")
    errs = _cached_steps_against_reforward(lm, B, 9, 3, cfg.vocab, seed=B)
    print(f"[{shape} B={B}] max |cached - re-forward| per step: {['%.3e' % e for e in errs]}")
    assert max(errs) <= TOL[torch.bfloat16]["logits"]


def test_fp32_cached_step_logits_match_the_reforward():
    """float32 takes the prefill sequence with Sq = 1 (eavqa_rope on one row per sample, append, attention over the cache)."""
    z = load_golden(FIXTURE)
    from eavqa_amd.models.lm import FrozenCausalLM
    cfg, _, _ = llama_config(z)
    lm = FrozenCausalLM(cfg, sub(z, "lm."), torch.float32, DEV)
    errs = _cached_steps_against_reforward(lm, 4, 9, 3, cfg.vocab, seed=1)
    assert max(errs) <= TOL[torch.float32]["logits"]


def test_generate_fewshot_three_images_cached_equals_reforward_fp32():
    z = load_golden(FIXTURE)
    model = build_model(z, torch.float32).eval()
    V = int(z["cfg"][0])
    D = int(z["cfg"][6])
    B, n_img, sentinel, pad = 3, 3, V - 1, int(z["pad_id"])
    g = torch.Generator().manual_seed(4)
    rows, mask = [], []
    for b in range(B):
        seg = []
        for _ in range(n_img):
            seg += [sentinel] + torch.randint(3, V - 2, (2 + b,), generator=g).tolist()
        rows.append(seg)
    T_ = max(len(r) for r in rows)
    tok = torch.full((B, T_), pad, dtype=torch.long)
    qm = torch.zeros(B, T_, dtype=torch.long)
    for b, r in enumerate(rows):
        tok[b, :len(r)] = torch.tensor(r)
        qm[b, :len(r)] = 1
    prefix = torch.randn(B, n_img, D, generator=g)
    kw = dict(question_tokens=tok, prefix=prefix, question_mask=qm, num_shots=n_img - 1, special_token_id=sentinel, max_length=4,
              pad_token_id=pad, eos_token_id=None)
    a = model.generate_fewshot(use_cache=True, **kw)
    b = model.generate_fewshot(use_cache=False, **kw)
    assert len(a) == B and all(len(r) == 4 for r in a)
    assert a == b


def test_searches_over_the_shared_prompt_step_are_refused_by_name():
    z = load_golden(FIXTURE)
    model = build_model(z, torch.float32).eval()
    kw = dict(question_tokens=T(z["gen_ids"]), prefix=T(z["prefix"]), question_mask=T(z["gen_mask"]), max_length=3, pad_token_id=int(z["pad_id"]))
    with pytest.raises(NotImplementedError, match="llama"):
        model.generate_beams(num_beams=2, **kw)
    with pytest.raises(NotImplementedError, match="llama"):
        model.generate_draws(num_return_sequences=2, seed=1, **kw)
    with pytest.raises(NotImplementedError, match="llama"):
        model.score_candidates(T(z["gen_ids"]), T(z["prefix"]), T(z["gen_mask"]), candidates=torch.tensor([[5, 6], [7, -100]]))


def test_block_driver_rejects_a_workspace_one_byte_short():
    from eavqa_amd import _lib, _lib_llama
    lib = _lib_llama.load()
    E, H, F, B = 256, 4, 704, 8
    table = (_lib_llama.LlamaLayer * 2)()
    for dtype, Sq in ((_lib.BF16, 1), (_lib.BF16, 9), (_lib.F32, 1)):
        need = int(lib.eavqa_llama_block_workspace_bytes(dtype, B * Sq, E, F))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        x = torch.zeros(B * Sq, E, device=DEV)
        pos = torch.zeros(B * Sq, dtype=torch.int32, device=DEV)
        tab = torch.zeros(16, (E // H) // 2, device=DEV)
        rc = lib.eavqa_llama_block_forward(dtype, 2, table, E, H, F, 1e-5, B, Sq, 0, 16, x.data_ptr(), pos.data_ptr(), tab.data_ptr(), tab.data_ptr(),
                                           16, None, 0, ws.data_ptr(), need - 1, None)
        assert rc == _lib.EAVQA_E_ARG
