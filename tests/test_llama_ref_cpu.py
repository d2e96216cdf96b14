"""CPU: tests/_llama_ref.py (the plain-torch Llama decoder the GPU tests and the golden generator lean on) against
``transformers.LlamaForCausalLM``, and the load-time expansion of grouped-query attention against the GQA model itself."""
import pytest
import torch

import _llama_ref

V, E, NLAY, NH, NKV, FFN, NPOS = 96, 64, 2, 4, 2, 96, 64


@pytest.fixture(scope="module")
def tiny():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(5)
    cfg = LlamaConfig(vocab_size=V, hidden_size=E, intermediate_size=FFN, num_hidden_layers=NLAY, num_attention_heads=NH,
                      num_key_value_heads=NKV, max_position_embeddings=NPOS, rms_norm_eps=1e-5, rope_theta=10000.0, tie_word_embeddings=False,
                      attention_bias=False, mlp_bias=False, attn_implementation="eager", pad_token_id=0, bos_token_id=1, eos_token_id=2)
    model = LlamaForCausalLM(cfg).eval()
    g = torch.Generator().manual_seed(6)
    B, S = 3, 11
    lens = torch.tensor([S, 7, 4])
    mask = (torch.arange(S)[None] < lens[:, None]).long()                   # right-padded rows
    emb = torch.randn(B, S, E, generator=g) * 0.5
    labels = torch.randint(3, V, (B, S), generator=g)
    labels[mask == 0] = -100
    return cfg, model, emb, mask, labels


def _hf(model, emb, mask, labels):
    S = emb.shape[1]
    with torch.no_grad():
        out = model(inputs_embeds=emb, attention_mask=mask, labels=labels, position_ids=torch.arange(S)[None].expand(emb.shape[0], S))
    return out.logits, out.loss


def test_the_restatement_equals_transformers_and_the_expanded_weights_equal_gqa(tiny):
    from transformers import LlamaConfig, LlamaForCausalLM
    from eavqa_amd.models.lm import pack_llama_qkv, rope_table
    cfg, model, emb, mask, labels = tiny
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    want_logits, want_loss = _hf(model, emb, mask, labels)
    rcfg = dict(n_layer=NLAY, n_head=NH, n_kv_head=NKV, eps=1e-5)
    table = rope_table(NPOS, E // NH, 10000.0)
    logits, loss = _llama_ref.forward(sd, rcfg, emb, mask, table, labels=labels)
    attended = mask != 0                                                     # a padded QUERY row is never read by anyone
    assert (logits - want_logits)[attended].abs().max().item() <= 1e-5
    assert abs(loss.item() - want_loss.item()) <= 1e-5
    # float64 agrees with float32 to float32 accuracy: the restatement is usable as a high-precision reference
    l64, _ = _llama_ref.forward(sd, rcfg, emb.double(), mask, table, labels=labels)
    assert (l64.float() - want_logits)[attended].abs().max().item() <= 1e-5

    # grouped-query attention expanded at load (the project's own packing function) is the same model: HF on the expanded weights
    mha_sd = _llama_ref.expand_gqa(sd, NLAY, NH, NKV, pack_llama_qkv)
    assert mha_sd["model.layers.0.self_attn.k_proj.weight"].shape == (E, E)
    mha_cfg = LlamaConfig(**{**cfg.to_dict(), "num_key_value_heads": NH})
    mha = LlamaForCausalLM(mha_cfg).eval()
    mha.load_state_dict(mha_sd)
    mha.config._attn_implementation = "eager"
    got_logits, got_loss = _hf(mha, emb, mask, labels)
    assert (got_logits - want_logits).abs().max().item() <= 1e-6
    assert abs(got_loss.item() - want_loss.item()) <= 1e-6
    # ... and so does the restatement told that every head has its own K / V
    r_logits, _ = _llama_ref.forward(mha_sd, dict(rcfg, n_kv_head=NH), emb, mask, table)
    assert (r_logits - logits).abs().max().item() <= 1e-6


def test_the_restatement_reproduces_the_reference_fixture(golden):
    """tests/golden/clipcap_llama_mlp.npz (the reference's own forward on a tiny HF Llama) from its stored weights and inputs: what the
    GPU tests compare the kernels with is what the restatement computes."""
    from eavqa_amd.models.lm import rope_table
    z = golden("clipcap_llama_mlp.npz")
    Vz, Ez, NL, H, NP, L, D, Fz, KV = [int(v) for v in z["cfg"]]
    T = lambda a: torch.from_numpy(a)
    sd = {k[3:]: T(v) for k, v in z.items() if k.startswith("lm.")}
    m = {k[4:]: T(v) for k, v in z.items() if k.startswith("map.")}
    pre = (torch.tanh(T(z["prefix"]) @ m["model.0.weight"].T + m["model.0.bias"]) @ m["model.2.weight"].T + m["model.2.bias"]).view(-1, L, Ez)
    emb = torch.cat([pre, sd["model.embed_tokens.weight"][T(z["ids"])]], dim=1)
    B = emb.shape[0]
    mask = torch.cat([torch.ones(B, L, dtype=torch.long), T(z["mask"])], dim=1)
    labels = torch.cat([torch.full((B, L), -100), T(z["labels"])], dim=1)
    table = rope_table(NP, Ez // H, float(z["rope_theta"]))
    logits, loss = _llama_ref.forward(sd, dict(n_layer=NL, n_head=H, n_kv_head=KV, eps=float(z["rms_norm_eps"])), emb, mask, table, labels=labels)
    assert (logits - T(z["logits"]))[mask != 0].abs().max().item() <= 1e-5
    assert abs(loss.item() - float(z["loss"])) <= 1e-5
    assert float(z["min_margin"]) >= 1e-3
