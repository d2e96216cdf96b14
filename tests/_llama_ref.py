"""A plain-torch restatement of the Llama decoder (HF ``LlamaForCausalLM``, transformers/models/llama/modeling_llama.py): RMSNorm,
rotate-half rotary positions from the project's own cos / sin table, grouped-query attention through ``repeat_kv``, SwiGLU, causal +
key-padding mask, shifted cross-entropy.  It runs in whatever dtype the weights are given in (float64 for references), reads HF's
state-dict names, and shares no code with the package under test beyond the table function it is given.  tests/test_llama_ref_cpu.py
pins it to transformers."""
import torch
import torch.nn.functional as F


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def rope(x, cos, sin):
    """x [B, H, S, hd]; cos / sin [S, hd / 2] (the half table: HF's is these columns twice)."""
    c = torch.cat([cos, cos], dim=-1).to(x.dtype)[None, None]
    s = torch.cat([sin, sin], dim=-1).to(x.dtype)[None, None]
    return x * c + rotate_half(x) * s


def rmsnorm(x, g, eps):
    return g * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def repeat_kv(x, n):
    B, Hk, S, hd = x.shape
    return x if n == 1 else x[:, :, None].expand(B, Hk, n, S, hd).reshape(B, Hk * n, S, hd)


def forward(sd, cfg, inputs_embeds, attention_mask, table, labels=None, position_ids=None):
    """``cfg``: dict(n_layer, n_head, n_kv_head, eps).  ``table``: (cos, sin) float32 [n_pos, hd / 2].  ``attention_mask`` [B, S]
    (1 = attended).  Returns (logits [B, S, V], loss or None) in the dtype of ``inputs_embeds``."""
    x = inputs_embeds
    dt = x.dtype
    B, S, E = x.shape
    H, Hk, eps = cfg["n_head"], cfg["n_kv_head"], cfg["eps"]
    hd = E // H
    w = lambda k: sd[k].to(dt)
    pos = torch.arange(S) if position_ids is None else position_ids
    cos, sin = table[0][pos].to(dt), table[1][pos].to(dt)
    allowed = torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None] & (attention_mask[:, None, None, :] != 0)
    bias = torch.zeros(B, 1, S, S, dtype=dt).masked_fill(~allowed, torch.finfo(dt).min)
    for i in range(cfg["n_layer"]):
        p = f"model.layers.{i}."
        a = rmsnorm(x, w(p + "input_layernorm.weight"), eps)
        q = (a @ w(p + "self_attn.q_proj.weight").T).view(B, S, H, hd).transpose(1, 2)
        k = (a @ w(p + "self_attn.k_proj.weight").T).view(B, S, Hk, hd).transpose(1, 2)
        v = (a @ w(p + "self_attn.v_proj.weight").T).view(B, S, Hk, hd).transpose(1, 2)
        q, k = rope(q, cos, sin), rope(k, cos, sin)
        k, v = repeat_kv(k, H // Hk), repeat_kv(v, H // Hk)
        att = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5 + bias, dim=-1)
        ctx = (att @ v).transpose(1, 2).reshape(B, S, E)
        x = x + ctx @ w(p + "self_attn.o_proj.weight").T
        a = rmsnorm(x, w(p + "post_attention_layernorm.weight"), eps)
        h = F.silu(a @ w(p + "mlp.gate_proj.weight").T) * (a @ w(p + "mlp.up_proj.weight").T)
        x = x + h @ w(p + "mlp.down_proj.weight").T
    x = rmsnorm(x, w("model.norm.weight"), eps)
    head = sd["lm_head.weight"] if "lm_head.weight" in sd else sd["model.embed_tokens.weight"]
    logits = x @ head.to(dt).T
    loss = None
    if labels is not None:
        loss = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1), ignore_index=-100)
    return logits, loss


def expand_gqa(sd, n_layer, n_head, n_kv_head, pack):
    """The state dict of the multi-head model that ``pack`` ([q; k; v] with K / V heads repeated) describes."""
    out = dict(sd)
    for i in range(n_layer):
        p = f"model.layers.{i}.self_attn."
        E = sd[p + "q_proj.weight"].shape[0]
        qkv = pack(sd[p + "q_proj.weight"], sd[p + "k_proj.weight"], sd[p + "v_proj.weight"], n_head, n_kv_head)
        out[p + "q_proj.weight"], out[p + "k_proj.weight"], out[p + "v_proj.weight"] = qkv[:E], qkv[E:2 * E], qkv[2 * E:]
    return out
