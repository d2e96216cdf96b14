"""CPU: the Llama family's configuration reader, its refusals, its named shapes and its rotary table (models/lm.py)."""
import os

import pytest
import torch

from eavqa_amd.models.lm import KNOWN_CONFIGS, LMConfig, random_init_state_dict, rope_table

BASE = dict(model_type="llama", hidden_size=128, intermediate_size=352, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
            rms_norm_eps=1e-5, rope_theta=500000.0, max_position_embeddings=512, vocab_size=1000, tie_word_embeddings=True, eos_token_id=7,
            pad_token_id=9, hidden_act="silu", attention_bias=False, mlp_bias=False, rope_scaling=None)


def test_fields_are_read():
    c = LMConfig.from_hf_dict(BASE)
    assert (c.arch, c.n_layer, c.n_head, c.n_embd, c.ffn, c.vocab, c.n_pos) == ("llama", 3, 8, 128, 352, 1000, 512)
    assert (c.eps, c.act, c.eos_token_id, c.pad_token_id) == (1e-5, "silu", 7, 9)
    assert (c.n_kv_head, c.kv_heads, c.rope_theta, c.tie_word_embeddings, c.head_dim, c.pos_mode) == (2, 2, 500000.0, True, 16, 0)
    assert LMConfig.from_hf_dict(dict(BASE, head_dim=16)).head_dim == 16


def test_defaults():
    d = {k: v for k, v in BASE.items() if k not in ("num_key_value_heads", "rope_theta", "tie_word_embeddings", "pad_token_id", "hidden_act",
                                                    "attention_bias", "mlp_bias", "rope_scaling")}
    c = LMConfig.from_hf_dict(d)
    assert c.n_kv_head == c.n_head == 8 and c.rope_theta == 10000.0 and c.pad_token_id is None and c.tie_word_embeddings is False


@pytest.mark.parametrize("change,key", [
    (dict(rope_scaling=dict(rope_type="linear", factor=2.0)), "rope_scaling"),
    (dict(attention_bias=True), "attention_bias"),
    (dict(mlp_bias=True), "mlp_bias"),
    (dict(hidden_act="gelu"), "hidden_act"),
    (dict(head_dim=32), "head_dim"),
    (dict(sliding_window=256), "sliding_window"),
    (dict(num_key_value_heads=3), "num_key_value_heads"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_refusals_name_the_key(change, key):
    with pytest.raises(NotImplementedError, match=key):
        LMConfig.from_hf_dict(dict(BASE, **change))


def test_fp8_weights_are_refused_for_the_family():
    from eavqa_amd.models.lm import FrozenCausalLM
    c = LMConfig.from_hf_dict(BASE)
    with pytest.raises(NotImplementedError, match="fp8"):
        FrozenCausalLM(c, {}, torch.bfloat16, "cpu", weight_format="fp8")


@pytest.mark.parametrize("theta", [1e4, 5e5])
@pytest.mark.parametrize("hd", [8, 64, 128])
def test_the_rotary_table_is_hf_s_bit_for_bit(hd, theta):
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    n_pos = 300
    cfg = LlamaConfig(hidden_size=4 * hd, num_attention_heads=4, num_hidden_layers=1, intermediate_size=32, vocab_size=32,
                      max_position_embeddings=n_pos, rope_theta=theta)
    rot = LlamaRotaryEmbedding(cfg)
    cos, sin = rot(torch.zeros(1, n_pos, 4 * hd), torch.arange(n_pos)[None])
    got_cos, got_sin = rope_table(n_pos, hd, theta)
    assert got_cos.dtype == torch.float32 and tuple(got_cos.shape) == (n_pos, hd // 2) and got_cos.is_contiguous()
    assert torch.equal(got_cos, cos[0, :, :hd // 2]) and torch.equal(got_cos, cos[0, :, hd // 2:])
    assert torch.equal(got_sin, sin[0, :, :hd // 2]) and torch.equal(got_sin, sin[0, :, hd // 2:])


def test_named_shapes_and_random_init():
    c = LMConfig.from_hf_dict(KNOWN_CONFIGS["meta-llama/Llama-2-7b-hf"])
    assert (c.n_embd, c.n_layer, c.n_head, c.kv_heads, c.ffn, c.vocab) == (4096, 32, 32, 32, 11008, 32000)
    t = LMConfig.from_hf_dict(KNOWN_CONFIGS["TinyLlama/TinyLlama-1.1B-Chat-v1.0"])
    assert (t.n_embd, t.n_layer, t.n_head, t.kv_heads, t.ffn, t.vocab) == (2048, 22, 32, 4, 5632, 32000)
    small = LMConfig.from_hf_dict(BASE)
    sd = random_init_state_dict(small, seed=1)
    assert sd["model.layers.2.self_attn.k_proj.weight"].shape == (2 * 16, 128) and sd["model.layers.0.mlp.gate_proj.weight"].shape == (352, 128)
    assert sd["model.layers.1.mlp.down_proj.weight"].shape == (128, 352) and sd["lm_head.weight"].shape == (1000, 128)
    assert not [k for k in sd if "bias" in k] and torch.equal(sd["model.norm.weight"], torch.ones(128))


def test_gpt2_and_opt_configs_are_unchanged():
    g = LMConfig.from_hf_dict(KNOWN_CONFIGS["gpt2"])
    assert (g.arch, g.n_layer, g.n_head, g.n_embd, g.ffn, g.vocab, g.n_pos, g.eps, g.act, g.eos_token_id, g.pad_token_id, g.pos_mode) == \
        ("gpt2", 12, 12, 768, 3072, 50257, 1024, 1e-5, "gelu_new", 50256, None, 0)
    o = LMConfig.from_hf_dict(KNOWN_CONFIGS["facebook/opt-2.7b"])
    assert (o.arch, o.n_layer, o.n_head, o.n_embd, o.ffn, o.vocab, o.n_pos, o.eps, o.act, o.eos_token_id, o.pad_token_id, o.pos_mode) == \
        ("opt", 32, 32, 2560, 10240, 50272, 2048, 1e-5, "relu", 2, 1, 1)
    p = LMConfig("opt", 2, 4, 64, 96, 336, 64, 1e-5, "relu", 2, 1)             # the positional form the suite uses
    assert (p.n_kv_head, p.kv_heads, p.rope_theta) == (None, 4, 10000.0)
    with pytest.raises(NotImplementedError, match="not a causal LM"):
        LMConfig.from_hf_dict(dict(model_type="mistral"))



def test_the_opt_few_shot_config_runs_a_llama_by_override():
    """No config file of its own: the few-shot config takes the LM by name, and an option override names a Llama shape."""
    import os
    from eavqa_amd.utils import config_system as cs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    few = cs.load_config(os.path.join(root, "configs", "vqa2", "few_shot_opt_2p7b.jsonnet"), mode="test",
                         opts=["model_config.model_args.model_version=meta-llama/Llama-2-7b-hf"])
    assert LMConfig.from_hf_dict(KNOWN_CONFIGS[dict(few.model_config.model_args)["model_version"]]).arch == "llama"


def test_the_second_library_exports_exactly_its_header():
    """libeavqa_llama_hip.so: the dynamic symbol table is the declarations of include/eavqa_llama.h, every one is bound, and the first
    library's header and table are not added to."""
    import re
    import subprocess
    from eavqa_amd import _lib, _lib_llama, build
    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(build.INCLUDE, "eavqa_llama.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(eavqa_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["eavqa_llama_block_forward", "eavqa_llama_block_workspace_bytes", "eavqa_rope", "eavqa_rope_finish", "eavqa_swiglu_bwd",
                        "eavqa_swiglu_fwd", "eavqa_swiglu_splitk"]
    out = subprocess.run(["nm", "-D", "--defined-only", build.LLAMA_LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == declared
    assert sorted(_lib_llama.SIGNATURES) == declared and not set(declared) & set(_lib.SIGNATURES)
    lib = _lib_llama.load()
    assert lib.eavqa_llama_block_workspace_bytes(1, 0, 64, 96) == 0 and lib.eavqa_llama_block_workspace_bytes(1, 4, 64, 96) > 0
    assert _lib_llama.SIGNATURES["eavqa_llama_block_forward"][2]._type_ is _lib_llama.LlamaLayer
    assert [n for n, _ in _lib_llama.LlamaLayer._fields_] == ["ln1_g", "w_qkv", "w_o", "ln2_g", "w_gu", "w_down", "k_cache", "v_cache"]
    assert len(_lib.STRUCTS) == 8                                            # the first library's structs are not added to
    assert lib.eavqa_rope(1, 4, 2, 12, 16, 128, 16, 16, 16, 32, 8, 0, None) == _lib.EAVQA_E_SHAPE      # rejected on the host, no launch
