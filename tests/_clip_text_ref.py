"""Plain-torch restatement of the CLIP text tower (HF ``CLIPTextModelWithProjection`` / OpenAI ``encode_text``): pre-LN layers, QuickGELU,
causal mask only, pooled at the arg-max of the ids.  float64 capable; tests/test_clip_text_ref_cpu.py pins it to the HF fixture."""
import torch
import torch.nn.functional as F


def encode_text_ref(sd, n_head, ids, eps=1e-5, dtype=torch.float64):
    W = {k: v.to(dtype) for k, v in sd.items()}
    p = "text_model."
    B, S = ids.shape
    x = W[p + "embeddings.token_embedding.weight"][ids] + W[p + "embeddings.position_embedding.weight"][:S][None]
    E = x.shape[-1]
    hd = E // n_head
    causal = torch.full((S, S), float("-inf"), dtype=dtype).triu(1)
    i = 0
    while f"{p}encoder.layers.{i}.layer_norm1.weight" in W:
        q = f"{p}encoder.layers.{i}."
        lin = lambda t, n: t @ W[q + n + ".weight"].T + W[q + n + ".bias"]
        a = F.layer_norm(x, (E,), W[q + "layer_norm1.weight"], W[q + "layer_norm1.bias"], eps)
        qq, kk, vv = (lin(a, "self_attn." + n + "_proj").view(B, S, n_head, hd).transpose(1, 2) for n in "qkv")
        att = torch.softmax(qq @ kk.transpose(-1, -2) * hd ** -0.5 + causal, dim=-1) @ vv
        x = x + lin(att.transpose(1, 2).reshape(B, S, E), "self_attn.out_proj")
        a = F.layer_norm(x, (E,), W[q + "layer_norm2.weight"], W[q + "layer_norm2.bias"], eps)
        h = lin(a, "mlp.fc1")
        x = x + lin(h * torch.sigmoid(1.702 * h), "mlp.fc2")
        i += 1
    pooled = x[torch.arange(B), ids.argmax(dim=1)]
    pooled = F.layer_norm(pooled, (E,), W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], eps)
    return pooled @ W["text_projection.weight"].T
