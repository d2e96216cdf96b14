"""CLIP text tower (``model.encode_text``) executed by the HIP kernels.

The reference calls OpenAI-CLIP's ``encode_text(clip.tokenize(question))`` offline, one question per call
(src/tools/extract_contrastive_text_embeddings.py:54-58), and stores the rows RICES searches
(src/in_context_example_selection/get_question_knn.py:64-76); this build runs the same arithmetic in batches.  Weights use
the HF ``CLIPTextModelWithProjection`` key names (``text_model.embeddings.{token,position}_embedding.weight``,
``text_model.encoder.layers.N.*``, ``text_model.final_layer_norm.*``, ``text_projection.weight``), which is the same graph as
OpenAI's text ``Transformer``: pre-LN layers, QuickGELU, causal attention and NO padding mask (OpenAI builds the causal mask only).

The interface starts at token ids.  The CLIP byte-pair tokeniser (its 49 408-entry vocabulary and merges file) is not part of
this package: ``encode_text`` takes what ``clip.tokenize`` returns, int [B, 77] rows ``<BOS> tokens <EOT> 0 0 ...``.

Packing.  The embedding of a row is read at ONE position, the arg-max of its ids (OpenAI: ``x[arange(B), text.argmax(dim=-1)]``,
the first EOT because EOT is the largest id), and under a causal mask nothing behind that position reaches it.  With ``pack=True``
(the default) every row is cut behind its EOT and the batch runs as ``cu_seqlens`` rows - a VQA question is about 10 of the 77
positions - and only the B pooled rows go through the final LayerNorm and the projection.  This is exact, not an approximation:
the kept positions see the same keys either way.  ``pack=False`` runs all 77 positions of every row.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import torch

from .. import ops

Tensor = torch.Tensor


@dataclass
class TextConfig:
    width: int
    n_layer: int
    n_head: int
    mlp: int
    proj: int
    context: int = 77
    vocab: int = 49408
    eps: float = 1e-5
    act: str = "quick_gelu"


KNOWN_TEXT_TOWERS = {
    "ViT-B/32": TextConfig(512, 12, 8, 2048, 512),
    "ViT-B/16": TextConfig(512, 12, 8, 2048, 512),
    "ViT-L/14": TextConfig(768, 12, 12, 3072, 768),
    "ViT-L/14@336px": TextConfig(768, 12, 12, 3072, 768),
}


def random_init_text_state_dict(cfg: TextConfig, seed: int = 2021, device="cpu") -> Dict[str, Tensor]:
    """Seeded random-init weights under HF key names (std 0.02-ish like HF's CLIP init; LayerNorm 1/0)."""
    g = torch.Generator(device=device).manual_seed(seed)
    W = cfg.width

    def n(*shape, std=0.02):
        return torch.randn(*shape, generator=g, device=device) * std

    ones, zeros = (lambda k: torch.ones(k, device=device)), (lambda k: torch.zeros(k, device=device))
    p = "text_model."
    sd = {
        p + "embeddings.token_embedding.weight": n(cfg.vocab, W),
        p + "embeddings.position_embedding.weight": n(cfg.context, W, std=0.01),
        p + "final_layer_norm.weight": ones(W), p + "final_layer_norm.bias": zeros(W),
        "text_projection.weight": n(cfg.proj, W, std=W ** -0.5),
    }
    for i in range(cfg.n_layer):
        q = f"{p}encoder.layers.{i}."
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[q + f"self_attn.{nm}.weight"], sd[q + f"self_attn.{nm}.bias"] = n(W, W, std=W ** -0.5), zeros(W)
        sd[q + "layer_norm1.weight"], sd[q + "layer_norm1.bias"] = ones(W), zeros(W)
        sd[q + "layer_norm2.weight"], sd[q + "layer_norm2.bias"] = ones(W), zeros(W)
        sd[q + "mlp.fc1.weight"], sd[q + "mlp.fc1.bias"] = n(cfg.mlp, W), zeros(cfg.mlp)
        sd[q + "mlp.fc2.weight"], sd[q + "mlp.fc2.bias"] = n(W, cfg.mlp), zeros(W)
    return sd


class ClipTextEncoder:
    """Frozen CLIP text transformer: ``encode_text(token_ids [B, context] int) -> float32 [B, proj]``.

    ``dtype``: ``torch.bfloat16`` (the MFMA kernels) or ``torch.float32`` (the parity path).  The residual stream is float32 in both
    modes.  ``pack``: cut every row behind its EOT (see the module docstring)."""

    MAX_BH = 65535                                    # eavqa_attention_fwd refuses B * H above this

    def __init__(self, cfg: TextConfig, state_dict: Dict[str, Tensor], dtype: torch.dtype = torch.bfloat16, device="cuda",
                 pack: bool = True):
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("dtype must be bfloat16 or float32")
        if cfg.width % cfg.n_head:
            raise ValueError("width must be a multiple of n_head")
        self.cfg, self.dtype, self.device, self.pack = cfg, dtype, torch.device(device), pack
        T = lambda t: t.to(device=self.device, dtype=dtype).contiguous()
        F = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()
        p = "text_model."
        self.wte = T(state_dict[p + "embeddings.token_embedding.weight"])
        self.wpe = T(state_dict[p + "embeddings.position_embedding.weight"])
        if self.wte.shape != (cfg.vocab, cfg.width) or self.wpe.shape != (cfg.context, cfg.width):
            raise ValueError("embedding tables do not match the config")
        self.final_g, self.final_b = F(state_dict[p + "final_layer_norm.weight"]), F(state_dict[p + "final_layer_norm.bias"])
        self.w_proj = T(state_dict["text_projection.weight"])
        self.layers = []
        for i in range(cfg.n_layer):
            q = f"{p}encoder.layers.{i}."
            self.layers.append(dict(
                ln1_g=F(state_dict[q + "layer_norm1.weight"]), ln1_b=F(state_dict[q + "layer_norm1.bias"]),
                w_qkv=T(torch.cat([state_dict[q + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)),
                b_qkv=F(torch.cat([state_dict[q + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)),
                w_o=T(state_dict[q + "self_attn.out_proj.weight"]), b_o=F(state_dict[q + "self_attn.out_proj.bias"]),
                ln2_g=F(state_dict[q + "layer_norm2.weight"]), ln2_b=F(state_dict[q + "layer_norm2.bias"]),
                w_fc1=T(state_dict[q + "mlp.fc1.weight"]), b_fc1=F(state_dict[q + "mlp.fc1.bias"]),
                w_fc2=T(state_dict[q + "mlp.fc2.weight"]), b_fc2=F(state_dict[q + "mlp.fc2.bias"]),
            ))

    @torch.no_grad()
    def encode_text(self, token_ids: Tensor, pack: bool = None) -> Tensor:
        """``token_ids``: int [B, context], on the host or on the GPU.  Rows go through the tower in chunks of at most
        ``MAX_BH // n_head`` (the attention kernels' grid limit); a row's embedding does not depend on its chunk."""
        c = self.cfg
        if token_ids.dim() != 2 or token_ids.shape[1] != c.context:
            raise ValueError(f"token_ids must be [B, {c.context}]")
        if token_ids.dtype.is_floating_point:
            raise ValueError("token_ids must be an integer tensor")
        pack = self.pack if pack is None else pack
        B = token_ids.shape[0]
        out = torch.empty((B, c.proj), device=self.device, dtype=torch.float32)
        step = self.MAX_BH // c.n_head
        for s in range(0, B, step):
            self._encode_chunk(token_ids[s:s + step], pack, out[s:s + step])
        return out

    def _encode_chunk(self, token_ids: Tensor, pack: bool, out: Tensor) -> None:
        c, T = self.cfg, self.dtype
        B, S = token_ids.shape
        W, H = c.width, c.n_head
        hd = W // H
        # lengths from a host tensor cost nothing; a device tensor costs this one read of B integers (the packed row count sizes
        # every buffer below).  Nothing else comes back from the device.
        eot_host = token_ids.argmax(dim=1) if pack and not token_ids.is_cuda else None
        ids = token_ids.to(device=self.device, dtype=torch.int64).contiguous()
        eot, cu, tok, pos, pooled = ops.clip_text_plan(ids, pack)
        if pack:
            if eot_host is None:
                eot_host = eot.cpu()
            M, smax, cu_arg = int(eot_host.sum()) + B, int(eot_host.max()) + 1, cu
        else:
            M, smax, cu_arg = B * S, S, None
        x = ops.embed_assemble(tok[:M], pos[:M], self.wte, None, self.wpe)       # float32 residual stream [M, W]
        x1 = torch.empty_like(x)
        for L in self.layers:
            a = ops.layernorm_fwd(x, L["ln1_g"], L["ln1_b"], c.eps, T)
            qkv = ops.gemm(a, L["w_qkv"], bias=L["b_qkv"])
            ctx = ops.attention_fwd(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], B, H, smax, smax, hd, causal=True, scale=hd ** -0.5,
                                    cu_seqlens=cu_arg)
            ops.gemm(ctx, L["w_o"], bias=L["b_o"], residual=x, out=x1)
            a2 = ops.layernorm_fwd(x1, L["ln2_g"], L["ln2_b"], c.eps, T)
            f = ops.gemm(a2, L["w_fc1"], bias=L["b_fc1"], act=c.act)
            ops.gemm(f, L["w_fc2"], bias=L["b_fc2"], residual=x1, out=x)
        rows = ops.gather_rows(x, pooled)                                       # the B pooled rows only
        final = ops.layernorm_fwd(rows, self.final_g, self.final_b, c.eps, T)
        ops.gemm(final, self.w_proj, out=out)
