"""Frozen causal LM (GPT-2 / OPT / Llama family) executed entirely by the HIP kernels.

Arithmetic mirrored:
  * GPT-2: HF ``GPT2LMHeadModel`` transformers/models/gpt2/modeling_gpt2.py:571-620 (positions =
    arange, wpe add), :246-309 (pre-LN block), :75-226 (c_attn Conv1D ``[in,out]``, scale hd^-0.5,
    causal + key-padding mask), :229-243 (gelu_new MLP), :698 (lm_head tied to wte);
  * OPT: HF ``OPTForCausalLM`` transformers/models/opt/modeling_opt.py:45-70 (learned positions,
    offset 2, ``cumsum(mask)*mask-1``), :97-181 (q scaled before q.k), :184-254 (pre-LN, ReLU),
    :273-397 (final_layer_norm), :443-538 (lm_head);
  * Llama family: HF ``LlamaForCausalLM`` transformers/models/llama/modeling_llama.py (LlamaRMSNorm; LlamaRotaryEmbedding +
    ``apply_rotary_pos_emb`` / ``rotate_half``; ``repeat_kv`` grouped-query attention; LlamaMLP ``down(silu(gate x) * up x)``; no biases;
    positions = arange when called with ``inputs_embeds`` and no ``position_ids``);
  * loss: transformers/loss/loss_utils.py:32-71 (shift, ignore -100, mean).

The LM is frozen (``ClipCaptionPrefix.train`` clipcap.py:594-599), so the backward pass is dgrad
only: no weight gradient and no GEMM input needs saving - only what the norms, attention and the
activation need.  The three families run ONE layer loop and ONE dgrad loop; what differs between them is data on the model, set where the
weights are packed: the norm (``lnf_b is None``: RMSNorm), ``rotary`` (q / k turned by position behind the QKV product, no learned
positions) and ``gated`` (SwiGLU feed-forward).  Weights are pre-packed once at load into the k-contiguous layouts the MFMA GEMM
streams fastest: a forward copy ``[N,K]`` and (lazily, for training) a backward copy ``[K,N]``;
288 GB of HBM makes the second copy free.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, NamedTuple, Optional

import torch

from .. import ops

Tensor = torch.Tensor


@dataclass
class LMConfig:
    arch: str            # "gpt2" | "opt" | "llama"
    n_layer: int
    n_head: int
    n_embd: int
    ffn: int
    vocab: int
    n_pos: int           # number of learned positions (OPT: excluding the offset of 2)
    eps: float = 1e-5
    act: str = "gelu_new"
    eos_token_id: Optional[int] = None
    pad_token_id: Optional[int] = None
    n_kv_head: Optional[int] = None      # llama: key / value heads of the checkpoint (None = n_head); expanded to n_head at load
    rope_theta: float = 10000.0          # llama: base of the rotary frequencies
    tie_word_embeddings: bool = True     # llama: no lm_head.weight in the checkpoint means "tied to embed_tokens"

    @property
    def head_dim(self) -> int:
        return self.n_embd // self.n_head

    @property
    def kv_heads(self) -> int:
        return self.n_kv_head if self.n_kv_head else self.n_head

    @property
    def pos_mode(self) -> int:
        # 0: pos[b, s] = s (GPT-2; Llama called with inputs_embeds and no position_ids); 1: OPT's cumsum(mask) - 1
        return 1 if self.arch == "opt" else 0

    @staticmethod
    def from_hf_dict(d: dict) -> "LMConfig":
        mt = d.get("model_type", "gpt2")
        if mt == "gpt2":
            E = d.get("n_embd", 768)
            return LMConfig("gpt2", d.get("n_layer", 12), d.get("n_head", 12), E, d.get("n_inner") or 4 * E,
                            d.get("vocab_size", 50257), d.get("n_positions", 1024), d.get("layer_norm_epsilon", 1e-5),
                            d.get("activation_function", "gelu_new"), d.get("eos_token_id", 50256), d.get("pad_token_id"))
        if mt == "opt":
            E = d.get("hidden_size", 768)
            if d.get("word_embed_proj_dim", E) != E or not d.get("do_layer_norm_before", True):
                raise NotImplementedError("OPT-350m style project_in/out / post-LN is not on the hot path")
            return LMConfig("opt", d.get("num_hidden_layers", 12), d.get("num_attention_heads", 12), E, d.get("ffn_dim", 3072),
                            d.get("vocab_size", 50272), d.get("max_position_embeddings", 2048), 1e-5,
                            d.get("activation_function", "relu"), d.get("eos_token_id", 2), d.get("pad_token_id", 1))
        if mt == "llama":
            return _llama_config(d)
        raise NotImplementedError(f"model_type {mt!r} is not a causal LM on the hot path")


def _llama_config(d: dict) -> LMConfig:
    """``LMConfig`` of an HF ``LlamaConfig`` dict.  What the kernels do not compute is refused by the name of its key."""
    E, H = d.get("hidden_size", 4096), d.get("num_attention_heads", 32)
    kv = d.get("num_key_value_heads") or H
    hd = d.get("head_dim") or E // H
    if d.get("rope_scaling") is not None:
        raise NotImplementedError(f"rope_scaling={d['rope_scaling']!r}: only the plain rotary table is on the hot path")
    for key in ("attention_bias", "mlp_bias"):
        if d.get(key):
            raise NotImplementedError(f"{key}=True: the Llama layer loop has no bias terms")
    if d.get("hidden_act", "silu") != "silu":
        raise NotImplementedError(f"hidden_act={d['hidden_act']!r}: the gated feed-forward is SwiGLU (silu) only")
    if hd * H != E:
        raise NotImplementedError(f"head_dim={hd}: head_dim * num_attention_heads must equal hidden_size ({E})")
    if d.get("sliding_window") is not None:
        raise NotImplementedError(f"sliding_window={d['sliding_window']!r}: only full causal attention is on the hot path")
    if H % kv:
        raise NotImplementedError(f"num_key_value_heads={kv} does not divide num_attention_heads={H}")
    return LMConfig("llama", d.get("num_hidden_layers", 32), H, E, d.get("intermediate_size", 11008), d.get("vocab_size", 32000),
                    d.get("max_position_embeddings", 2048), d.get("rms_norm_eps", 1e-6), "silu", d.get("eos_token_id", 2), d.get("pad_token_id"),
                    n_kv_head=kv, rope_theta=float(d.get("rope_theta", 10000.0)), tie_word_embeddings=bool(d.get("tie_word_embeddings", False)))


def rope_table(n_pos: int, head_dim: int, theta: float):
    """``(cos, sin)`` float32 [n_pos, head_dim / 2] on the host, computed as HF's ``LlamaRotaryEmbedding`` computes them (default rope
    type, float32): the kernels read this table and evaluate no sine themselves.  HF's table repeats these columns twice along the head."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))
    freqs = torch.arange(n_pos, dtype=torch.int64).float()[:, None] * inv_freq[None, :]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def pack_llama_qkv(q: Tensor, k: Tensor, v: Tensor, n_head: int, n_kv_head: int) -> Tensor:
    """``[q; k; v]`` [3E, E] of one layer with grouped-query attention expanded: every K / V head's projection rows are repeated
    ``n_head // n_kv_head`` times (``repeat_interleave`` over the head axis), which is what HF's ``repeat_kv`` does to the activations, so
    the kernels see plain multi-head attention and compute the same numbers."""
    g = n_head // n_kv_head
    if g > 1:
        hd = q.shape[0] // n_head
        k, v = (w.view(n_kv_head, hd, -1).repeat_interleave(g, dim=0).reshape(n_head * hd, -1) for w in (k, v))
    return torch.cat([q, k, v], dim=0)


# named model shapes used by BASELINE.json configs (public architecture constants)
KNOWN_CONFIGS = {
    "gpt2": dict(model_type="gpt2", n_embd=768, n_layer=12, n_head=12, vocab_size=50257, n_positions=1024),
    "gpt2-medium": dict(model_type="gpt2", n_embd=1024, n_layer=24, n_head=16, vocab_size=50257, n_positions=1024),
    "gpt2-large": dict(model_type="gpt2", n_embd=1280, n_layer=36, n_head=20, vocab_size=50257, n_positions=1024),
    "gpt2-xl": dict(model_type="gpt2", n_embd=1600, n_layer=48, n_head=25, vocab_size=50257, n_positions=1024),
    "facebook/opt-125m": dict(model_type="opt", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, ffn_dim=3072),
    "facebook/opt-1.3b": dict(model_type="opt", hidden_size=2048, num_hidden_layers=24, num_attention_heads=32, ffn_dim=8192),
    "facebook/opt-2.7b": dict(model_type="opt", hidden_size=2560, num_hidden_layers=32, num_attention_heads=32, ffn_dim=10240),
    "facebook/opt-6.7b": dict(model_type="opt", hidden_size=4096, num_hidden_layers=32, num_attention_heads=32, ffn_dim=16384),
    "meta-llama/Llama-2-7b-hf": dict(model_type="llama", hidden_size=4096, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32,
                                     intermediate_size=11008, vocab_size=32000, max_position_embeddings=4096, rms_norm_eps=1e-5,
                                     bos_token_id=1, eos_token_id=2),
    "TinyLlama/TinyLlama-1.1B-Chat-v1.0": dict(model_type="llama", hidden_size=2048, num_hidden_layers=22, num_attention_heads=32,
                                               num_key_value_heads=4, intermediate_size=5632, vocab_size=32000, max_position_embeddings=2048,
                                               rms_norm_eps=1e-5, bos_token_id=1, eos_token_id=2),
}


def random_init_state_dict(cfg: LMConfig, seed: int = 2021, device="cpu") -> Dict[str, Tensor]:
    """Seeded random-init weights in HF key names / HF shapes (normal(0, 0.02), LayerNorm 1/0,
    zero biases; GPT-2 c_proj scaled by 1/sqrt(2*n_layer) as HF ``_init_weights`` does).  Used for
    synthetic benchmarks - there are no pretrained weights offline."""
    g = torch.Generator(device=device).manual_seed(seed)
    E, F, V = cfg.n_embd, cfg.ffn, cfg.vocab

    def n(*shape, std=0.02):
        return torch.randn(*shape, generator=g, device=device) * std

    sd: Dict[str, Tensor] = {}
    ones, zeros = (lambda k: torch.ones(k, device=device)), (lambda k: torch.zeros(k, device=device))
    if cfg.arch == "gpt2":
        sd["transformer.wte.weight"] = n(V, E)
        sd["transformer.wpe.weight"] = n(cfg.n_pos, E)
        ps = 0.02 / math.sqrt(2 * cfg.n_layer)
        for i in range(cfg.n_layer):
            p = f"transformer.h.{i}."
            sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = ones(E), zeros(E)
            sd[p + "attn.c_attn.weight"], sd[p + "attn.c_attn.bias"] = n(E, 3 * E), zeros(3 * E)
            sd[p + "attn.c_proj.weight"], sd[p + "attn.c_proj.bias"] = n(E, E, std=ps), zeros(E)
            sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = ones(E), zeros(E)
            sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = n(E, F), zeros(F)
            sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = n(F, E, std=ps), zeros(E)
        sd["transformer.ln_f.weight"], sd["transformer.ln_f.bias"] = ones(E), zeros(E)
    elif cfg.arch == "llama":
        kvE = cfg.kv_heads * cfg.head_dim
        sd["model.embed_tokens.weight"] = n(V, E)
        for i in range(cfg.n_layer):
            p = f"model.layers.{i}."
            sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = ones(E), ones(E)
            sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.o_proj.weight"] = n(E, E), n(E, E)
            sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"] = n(kvE, E), n(kvE, E)
            sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = n(F, E), n(F, E), n(E, F)
        sd["model.norm.weight"] = ones(E)
        sd["lm_head.weight"] = n(V, E)
    else:
        pre = "model.decoder."
        sd[pre + "embed_tokens.weight"] = n(V, E)
        sd[pre + "embed_positions.weight"] = n(cfg.n_pos + 2, E)
        for i in range(cfg.n_layer):
            p = f"{pre}layers.{i}."
            for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
                sd[p + f"self_attn.{nm}.weight"], sd[p + f"self_attn.{nm}.bias"] = n(E, E), zeros(E)
            sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"] = ones(E), zeros(E)
            sd[p + "fc1.weight"], sd[p + "fc1.bias"] = n(F, E), zeros(F)
            sd[p + "fc2.weight"], sd[p + "fc2.bias"] = n(E, F), zeros(E)
            sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"] = ones(E), zeros(E)
        sd[pre + "final_layer_norm.weight"], sd[pre + "final_layer_norm.bias"] = ones(E), zeros(E)
    return sd


def synthetic_weights_notice(model_version: str) -> None:
    """A known architecture NAME without a local HF directory gets seeded random-init weights (there is no network): say so once per
    name, loudly - answers and losses from such a model mean nothing - and refuse outright under ``EAVQA_REQUIRE_PRETRAINED=1``."""
    if os.environ.get("EAVQA_REQUIRE_PRETRAINED", "0") == "1":
        raise FileNotFoundError(f"{model_version!r}: no local HF directory (EAVQA_MODEL_DIR) and EAVQA_REQUIRE_PRETRAINED=1 forbids "
                                "the seeded random-init stand-in")
    import warnings
    warnings.warn(f"{model_version!r} is not a local HF directory: using SEEDED RANDOM-INIT weights of that architecture (synthetic runs "
                  "only; set EAVQA_MODEL_DIR to a directory of HF checkpoints, or EAVQA_REQUIRE_PRETRAINED=1 to make this an error)",
                  RuntimeWarning, stacklevel=3)


def load_local_hf(path: str):
    """(config dict, state dict) from a local HF directory: safetensors, else a torch file loaded
    with ``weights_only=True``.  Nothing is fetched from the network."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return cfg, load_file(st)
    pt = os.path.join(path, "pytorch_model.bin")
    if os.path.exists(pt):
        return cfg, torch.load(pt, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {path}")


class Fp8Weight:
    """A frozen Linear weight ``[N, K]`` held as OCP e4m3 bytes with ONE float scale (``w ~ scale * e4m3``): BASELINE
    configs[4].  ``t()`` is the transposed copy for the dgrad GEMM - the same bytes transposed, the same scale."""

    __slots__ = ("q", "scale", "shape")

    def __init__(self, q: Tensor, scale: float):
        self.q, self.scale, self.shape = q, float(scale), tuple(q.shape)

    @staticmethod
    def quantize(w: Tensor, device) -> "Fp8Weight":
        w = w.to(device=device, dtype=torch.float32)
        amax = float(w.abs().max().item())
        scale = amax / 448.0 if amax > 0 else 1.0
        q = (w / scale).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()      # load-time cast (torch), not on the hot path
        return Fp8Weight(q, scale)

    def t(self) -> "Fp8Weight":
        return Fp8Weight(self.q.T.contiguous(), self.scale)

    def dequantize(self) -> Tensor:
        return self.q.view(torch.float8_e4m3fn).float() * self.scale


def linear(a: Tensor, w, **kw) -> Tensor:
    """``epilogue(a @ w^T)``: the bf16 / fp32 MFMA GEMM, or - for an :class:`Fp8Weight` - row-wise e4m3 quantisation of ``a``
    followed by the block-scaled fp8 GEMM (eavqa_quantize_rows_fp8 + eavqa_gemm_fp8)."""
    if isinstance(w, Fp8Weight):
        kw.pop("prefetch", None)                            # (the fp8 kernels carry no look-ahead)
        # (a producer that already quantised its rows - eavqa_layernorm_fwd_fp8 / _bwd_fp8 - hands over the pair)
        aq, a_scale = a if isinstance(a, tuple) else ops.quantize_rows_fp8(a)
        return ops.gemm_fp8(aq, a_scale, w.q, w.scale, **kw)
    return ops.gemm(a, w, **kw)


def _attention(q: Tensor, k: Tensor, v: Tensor, *dims, save_lse: bool, **kw):
    """``ops.attention_fwd`` -> ``(ctx, lse)``, ``lse`` None unless ``save_lse``."""
    r = ops.attention_fwd(q, k, v, *dims, save_lse=save_lse, **kw)
    return r if save_lse else (r, None)


def _no_hint(w):
    return None


class RowPlan(NamedTuple):
    """The rows of one pass (:meth:`FrozenCausalLM._row_plan`): with packing ``cu`` [B + 1] row offsets, the packed ``src`` / ``pos`` /
    ``flat`` (row -> b * S + s) / ``row_labels`` cut to ``M`` rows and no key mask; without, the [B, S] inputs and ``attn_mask``."""
    cu: Optional[Tensor]
    src: Tensor
    pos: Tensor
    flat: Optional[Tensor]
    row_labels: Optional[Tensor]
    M: int
    attn_mask: Optional[Tensor]


class LayerTape(NamedTuple):
    """What one layer's dgrad needs from its forward: the stream in front of the layer (``x``) and behind the attention block (``x1``),
    the statistics of ln_1 / ln_2 (RMSNorm: the means None), the QKV rows (rotary: q and k AFTER the rotation, what the attention
    backward differentiates), the attention output and log-sum-exp, the activation's input ``u`` (gated: the gate | up rows)."""
    x: Tensor
    mean1: Tensor
    rstd1: Tensor
    qkv: Tensor
    ctx: Tensor
    lse: Tensor
    x1: Tensor
    mean2: Tensor
    rstd2: Tensor
    u: Tensor


class Tape(NamedTuple):
    """``out["tape"]`` of a training forward, read by :meth:`FrozenCausalLM.backward`."""
    layers: List[LayerTape]
    x_last: Tensor
    meanf: Tensor
    rstdf: Tensor
    logits: Tensor
    labels: Tensor
    sel: Optional[Tensor]
    row_lse: Tensor
    count: Tensor
    src: Tensor
    mask: Optional[Tensor]
    cu: Optional[Tensor]
    B: int
    S: int
    M: int
    pos: Optional[Tensor] = None      # the position of every row (a rotary model's backward turns dq / dk back by it)


class _Layer:
    __slots__ = ("ln1_g", "ln1_b", "w_qkv", "b_qkv", "w_o", "b_o", "ln2_g", "ln2_b", "w_fc1", "b_fc1", "w_fc2", "b_fc2",
                 "w_qkv_t", "w_o_t", "w_fc1_t", "w_fc2_t",
                 "w_qkv_f", "c_qkv", "d_qkv", "w_fc1_f", "c_fc1", "d_fc1")      # LayerNorm folded into the consuming Linear (_prepare_fold)


class FrozenCausalLM:
    """Weights of a frozen GPT-2 / OPT / Llama-family decoder pre-packed for the HIP kernels + forward / dgrad drivers."""

    def __init__(self, cfg: LMConfig, state_dict: Dict[str, Tensor], dtype: torch.dtype = torch.bfloat16, device="cuda",
                 weight_format: str = "native"):
        """``weight_format="fp8"`` (with ``dtype=torch.bfloat16``): the Linear weights of every layer and the lm_head are held
        in e4m3 with per-tensor scales and multiplied on the block-scaled MFMA; activations stay bf16 in HBM and are quantised
        row-wise right in front of each GEMM; LayerNorm, attention, the residual stream (fp32) and the loss are unchanged."""
        self.cfg = cfg
        self.dtype = dtype
        self.device = torch.device(device)
        if weight_format not in ("native", "fp8"):
            raise ValueError("weight_format must be 'native' or 'fp8'")
        if weight_format == "fp8" and cfg.arch == "llama":
            raise NotImplementedError('weight_format="fp8" with arch="llama": the e4m3 routes are built for GPT-2 / OPT layers')
        if weight_format == "fp8" and (dtype != torch.bfloat16 or cfg.n_embd % 128 or cfg.ffn % 128):
            raise ValueError("fp8 weights need bfloat16 activations and n_embd / ffn multiples of 128")
        self.weight_format = weight_format
        self._pack(state_dict)
        self._bwd_ready = False
        # eavqa_gemm_ln: ln_1 / ln_2 of layers 1.. (and ln_2 of layer 0) as an epilogue term of the QKV / FFN-up products instead of a
        # kernel of their own - bf16 weights only.  Measured equal to the LayerNorm kernels on cfg2 (what the 72 removed launches save, the
        # four longer GEMM epilogues per layer cost: profiles/round4_ln_fold.md), so it is an option (EAVQA_LN_FOLD=1), not the default.
        # What it folds is a LayerNorm: an RMSNorm family never takes the route.
        self.fold_layernorm = (self.lnf_b is not None and dtype == torch.bfloat16 and weight_format == "native"
                               and os.environ.get("EAVQA_LN_FOLD", "0") == "1")
        self._fold_ready = False
        # eavqa_gemm_pf: every GEMM names the weight matrix of the NEXT one in program order, whose lines its loader waves touch so that the
        # matrix waits in the Infinity Cache (in a step every weight is cold: 2.8 GB of them pass between two uses).  bf16 native weights, not
        # the fold_layernorm route (eavqa_gemm_ln takes no region).  EAVQA_WEIGHT_PREFETCH=0 turns the hints off for an A / B run
        # (profiles/weight_prefetch.md).
        self.weight_prefetch = (dtype == torch.bfloat16 and weight_format == "native" and os.environ.get("EAVQA_WEIGHT_PREFETCH", "1") != "0")
        # e4m3 weights: ln_1 / ln_2 (forward) and the LayerNorm backward hand their result to the next Linear already row-quantised
        # (EAVQA_FUSE_QUANT=0 keeps the separate eavqa_quantize_rows_fp8 launches: same bytes, the A / B switch)
        self.fuse_quantizer = os.environ.get("EAVQA_FUSE_QUANT", "1") != "0"

    # ---------------------------------------------------------------- packing
    def _T(self, t: Tensor) -> Tensor:
        return t.to(device=self.device, dtype=self.dtype).contiguous()

    def _F(self, t: Tensor) -> Tensor:
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _pack(self, sd: Dict[str, Tensor]) -> None:
        c = self.cfg
        self.layers = []
        self.rotary = self.gated = False      # (with ``lnf_b is None`` for RMSNorm: all the layer loop and the dgrad loop ask about a family)
        if c.arch == "gpt2":
            self.wte = self._T(sd["transformer.wte.weight"])
            self.wpe = self._T(sd["transformer.wpe.weight"])
            for i in range(c.n_layer):
                p = f"transformer.h.{i}."
                L = _Layer()
                L.ln1_g, L.ln1_b = self._F(sd[p + "ln_1.weight"]), self._F(sd[p + "ln_1.bias"])
                # Conv1D stores [in,out]; the forward GEMM wants [out,in] (k contiguous)
                L.w_qkv, L.b_qkv = self._T(sd[p + "attn.c_attn.weight"].T), self._F(sd[p + "attn.c_attn.bias"])
                L.w_o, L.b_o = self._T(sd[p + "attn.c_proj.weight"].T), self._F(sd[p + "attn.c_proj.bias"])
                L.ln2_g, L.ln2_b = self._F(sd[p + "ln_2.weight"]), self._F(sd[p + "ln_2.bias"])
                L.w_fc1, L.b_fc1 = self._T(sd[p + "mlp.c_fc.weight"].T), self._F(sd[p + "mlp.c_fc.bias"])
                L.w_fc2, L.b_fc2 = self._T(sd[p + "mlp.c_proj.weight"].T), self._F(sd[p + "mlp.c_proj.bias"])
                L.w_qkv_t = L.w_o_t = L.w_fc1_t = L.w_fc2_t = None
                self.layers.append(L)
            self.lnf_g, self.lnf_b = self._F(sd["transformer.ln_f.weight"]), self._F(sd["transformer.ln_f.bias"])
            head = sd.get("lm_head.weight")
        elif c.arch == "llama":
            # RMSNorm and no biases: the *_b fields stay None; w_fc1 = [gate; up] (the layout of eavqa_gated_act_* / eavqa_swiglu_*), w_fc2 =
            # down.  No learned positions: the rotary table instead.
            self.wte, self.wpe = self._T(sd["model.embed_tokens.weight"]), None
            for i in range(c.n_layer):
                p = f"model.layers.{i}."
                L = _Layer()
                L.ln1_g, L.ln2_g = self._F(sd[p + "input_layernorm.weight"]), self._F(sd[p + "post_attention_layernorm.weight"])
                L.ln1_b = L.ln2_b = L.b_qkv = L.b_o = L.b_fc1 = L.b_fc2 = None
                L.w_qkv = self._T(pack_llama_qkv(*(sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"), c.n_head, c.kv_heads))
                L.w_o = self._T(sd[p + "self_attn.o_proj.weight"])
                L.w_fc1 = self._T(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], dim=0))
                L.w_fc2 = self._T(sd[p + "mlp.down_proj.weight"])
                L.w_qkv_t = L.w_o_t = L.w_fc1_t = L.w_fc2_t = None
                self.layers.append(L)
            self.lnf_g, self.lnf_b = self._F(sd["model.norm.weight"]), None
            cos, sin = rope_table(c.n_pos, c.head_dim, c.rope_theta)
            self.rope_cos, self.rope_sin = self._F(cos), self._F(sin)
            self.rotary = self.gated = True
            head = sd.get("lm_head.weight")
        else:
            pre = "model.decoder."
            self.wte = self._T(sd[pre + "embed_tokens.weight"])
            self.wpe = self._T(sd[pre + "embed_positions.weight"])
            for i in range(c.n_layer):
                p = f"{pre}layers.{i}."
                L = _Layer()
                L.ln1_g, L.ln1_b = self._F(sd[p + "self_attn_layer_norm.weight"]), self._F(sd[p + "self_attn_layer_norm.bias"])
                L.w_qkv = self._T(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], dim=0))
                L.b_qkv = self._F(torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], dim=0))
                L.w_o, L.b_o = self._T(sd[p + "self_attn.out_proj.weight"]), self._F(sd[p + "self_attn.out_proj.bias"])
                L.ln2_g, L.ln2_b = self._F(sd[p + "final_layer_norm.weight"]), self._F(sd[p + "final_layer_norm.bias"])
                L.w_fc1, L.b_fc1 = self._T(sd[p + "fc1.weight"]), self._F(sd[p + "fc1.bias"])
                L.w_fc2, L.b_fc2 = self._T(sd[p + "fc2.weight"]), self._F(sd[p + "fc2.bias"])
                L.w_qkv_t = L.w_o_t = L.w_fc1_t = L.w_fc2_t = None
                self.layers.append(L)
            self.lnf_g, self.lnf_b = self._F(sd[pre + "final_layer_norm.weight"]), self._F(sd[pre + "final_layer_norm.bias"])
            head = sd.get("lm_head.weight")
        # lm_head is tied to wte in both families; an untied head is kept separately
        self.head = self.wte if head is None or head.shape == self.wte.shape and _same(head, self.wte) else self._T(head)
        self.head_t = None
        self.head_q = None
        if self.fp8:
            for L in self.layers:
                for name in ("w_qkv", "w_o", "w_fc1", "w_fc2"):
                    setattr(L, name, Fp8Weight.quantize(getattr(L, name), self.device))
            self.head_q = Fp8Weight.quantize(self.head, self.device)      # the bf16 wte stays for the embedding gather

    # a matrix beyond a quarter of the 256 MiB Infinity Cache (the lm_head of a 50k vocabulary: 129 MB) would push out what the kernels in
    # between still need, and its own head would be gone before its tail arrives: no hint
    PREFETCH_MAX_BYTES = 64 << 20

    def _hint(self, w):
        """``w`` as the ``prefetch=`` argument of the GEMM that runs before the one that streams it (None: no hint)."""
        if not self.weight_prefetch or not isinstance(w, torch.Tensor) or w.numel() * w.element_size() > self.PREFETCH_MAX_BYTES:
            return None
        return w

    @property
    def fp8(self) -> bool:
        """The Linear weights are held in e4m3 (``weight_format="fp8"``)."""
        return self.weight_format == "fp8"

    @property
    def vocab(self) -> int:
        return self.wte.shape[0]

    @property
    def vpad(self) -> int:
        q = 128 if self.fp8 else 64
        return (self.vocab + q - 1) // q * q   # K of the lm_head dgrad GEMM: a multiple of the kernels' K-step

    def _prepare_backward(self) -> None:
        """Transposed weight copies for the dgrad GEMMs (made once, on the first training step)."""
        if self._bwd_ready:
            return
        tr = (lambda w: w.t()) if self.fp8 else (lambda w: w.T.contiguous())
        for L in self.layers:
            L.w_qkv_t = tr(L.w_qkv)
            L.w_o_t = tr(L.w_o)
            L.w_fc1_t = tr(L.w_fc1)
            L.w_fc2_t = tr(L.w_fc2)
        V, E = self.head.shape
        if self.fp8:
            qt = torch.zeros((E, self.vpad), device=self.device, dtype=torch.uint8)      # e4m3 zero = byte 0
            qt[:, :V] = self.head_q.q.T
            self.head_t = Fp8Weight(qt, self.head_q.scale)
        else:
            self.head_t = torch.zeros((E, self.vpad), device=self.device, dtype=self.dtype)
            self.head_t[:, :V] = self.head.T
        self._bwd_ready = True

    def _prepare_fold(self) -> None:
        """``LayerNorm(x) W^T + b = rstd (x W'^T - mean c) + d`` with ``W' = W * gamma``, ``c = W' 1``, ``d = W beta + b`` (include/eavqa.h,
        eavqa_gemm_ln): the folded copies of the two weights of every layer that follow a LayerNorm, made once on the first training /
        scoring forward.  ``c`` sums W' AS STORED (bf16), so the rank-1 term cancels the mean of exactly the product the kernel forms."""
        if self._fold_ready:
            return
        for L in self.layers:
            for w, b, g, be, nm in ((L.w_qkv, L.b_qkv, L.ln1_g, L.ln1_b, "qkv"), (L.w_fc1, L.b_fc1, L.ln2_g, L.ln2_b, "fc1")):
                w32 = w.float()
                wf = (w32 * g[None, :]).to(self.dtype).contiguous()
                setattr(L, f"w_{nm}_f", wf)
                setattr(L, f"c_{nm}", wf.float().sum(1).contiguous())
                setattr(L, f"d_{nm}", (w32 @ be + b).contiguous())
                del w32
        self._fold_ready = True

    def resize_token_embeddings(self, n: int) -> None:
        """``model.gpt.resize_token_embeddings(len(tokenizer))`` src/trainers/clipcap_exector.py:56.
        New rows get the mean of the existing embeddings (HF draws them around that mean)."""
        V, E = self.wte.shape
        if n == V:
            return
        tied = self.head is self.wte
        new = torch.empty((n, E), device=self.device, dtype=self.dtype)
        keep = min(n, V)
        new[:keep] = self.wte[:keep]
        if n > V:
            new[V:] = self.wte.float().mean(0).to(self.dtype)
        self.wte = new
        if tied:
            self.head = new
        else:
            h = torch.empty((n, E), device=self.device, dtype=self.dtype)
            h[:keep] = self.head[:keep]
            if n > V:
                h[V:] = self.head.float().mean(0).to(self.dtype)
            self.head = h
        self.cfg.vocab = n
        self._bwd_ready = False
        if self.fp8:
            self.head_q = Fp8Weight.quantize(self.head, self.device)

    def load_token_embeddings(self, weight: Tensor) -> None:
        """Replace the token embedding matrix (and the tied head) by ``weight`` [vocab, E] - e.g. the rows a reference
        checkpoint holds after its ``resize_token_embeddings`` drew the new ones at random."""
        if tuple(weight.shape) != tuple(self.wte.shape):
            raise ValueError(f"token embedding shape {tuple(weight.shape)} does not match {tuple(self.wte.shape)}")
        tied = self.head is self.wte
        self.wte = self._T(weight)
        if tied:
            self.head = self.wte
        self._bwd_ready = False
        if self.fp8:
            self.head_q = Fp8Weight.quantize(self.head, self.device)

    # ---------------------------------------------------------------- forward
    def forward(self, prefix_rows: Optional[Tensor], src: Tensor, pos: Tensor, mask: Tensor, B: int, S: int, *,
                labels: Optional[Tensor] = None, save: bool = False, logits: str = "none", pack: bool = False,
                lengths=None, n_scored: Optional[int] = None):
        """Run the decoder over ``B`` rows of ``S`` positions.

        ``src/pos/mask``: int32 [B,S] from ``ops.build_prefix_rows`` / ``build_fewshot_rows``;
        ``prefix_rows``: mapper output rows in the compute dtype.  ``logits``: "none" | "all" | "last".
        ``pack``: drop the padded positions (mask == 0) before the first GEMM (``eavqa_build_row_plan``): the loss
        and every attended position are unchanged, the work shrinks from B*S to sum(lengths) rows.  ``lengths``
        (host ints, attended positions per sample) saves the one device->host read of the packed row count.
        Returns a dict with ``loss``/``count`` (when labels), ``logits`` ([rows or B, vpad] fp32; with ``pack`` also
        ``flat_index`` mapping packed rows to b*S+s) and, when ``save``, the tape for :meth:`backward`.
        ``n_scored`` (host int, with ``pack`` and ``labels``): the number of positions that carry a label - exactly
        ``(labels != -100).sum()`` when every label has a predecessor position, as behind a prefix; the collate has it on
        the host.  Then only those rows go through the lm_head and its dgrad (``out["logits"]`` holds just them, ``sel``
        their packed row numbers).
        """
        c = self.cfg
        E, H, hd = c.n_embd, c.n_head, c.head_dim
        scale = hd ** -0.5
        plan = self._row_plan(src, pos, mask, B, S, labels, pack, lengths)
        M = plan.M
        x = ops.embed_assemble(plan.src, plan.pos, self.wte, prefix_rows, self.wpe)

        def attend(li, q, k, v):
            return _attention(q, k, v, B, H, S, S, hd, key_mask=plan.attn_mask, causal=True, scale=scale, save_lse=save, cu_seqlens=plan.cu)

        pos_rows = plan.pos.reshape(-1)
        if self.fold_layernorm and M > 64:
            x, layers = self.layer_loop_folded(x, attend, save)
        else:
            x, layers = self.layer_loop(x, attend, save, hints=True, pos=pos_rows)
        out = {"rows": M, "flat_index": plan.flat}
        if logits == "last" and labels is None and not pack:
            out["logits"] = self._head(self.final_norm(x.view(B, S, E)[:, -1]))      # strided rows: only the last position is normalised
            return out
        hf, meanf, rstdf = self._norm(x, self.lnf_g, self.lnf_b, save, quantize=False)
        out["hidden"] = hf
        if labels is not None or logits == "all":
            sel = sel_count = None
            if pack and labels is not None and n_scored is not None and logits != "all" and 0 < n_scored < M:
                sel, ce_labels, sel_count = ops.select_rows(plan.row_labels, int(n_scored))
                lg = self._head(ops.gather_rows(hf, sel))
            else:
                lg = self._head(hf)
                ce_labels = plan.row_labels if pack else labels
            out["logits"], out["sel"] = lg, sel
            if labels is not None:
                loss, count, row_lse = ops.ce_fwd(lg, ce_labels, self.vocab)
                if sel_count is not None:
                    # the host-side label count sized the compaction: more labelled rows than that would have been dropped
                    # silently, so the loss turns NaN instead (on the device, no synchronisation)
                    ops.guard_count(sel_count, int(n_scored), loss)
                out["loss"], out["count"] = loss, count
                if save:
                    out["tape"] = Tape(layers=layers, x_last=x, meanf=meanf, rstdf=rstdf, logits=lg, labels=ce_labels, sel=sel,
                                       row_lse=row_lse, count=count, src=plan.src, mask=plan.attn_mask, cu=plan.cu, B=B, S=S, M=M, pos=pos_rows)
        return out

    def _row_plan(self, src: Tensor, pos: Tensor, mask: Tensor, B: int, S: int, labels: Optional[Tensor], pack: bool, lengths) -> RowPlan:
        """The rows a pass runs over: all B * S positions under the key mask, or (``pack``) the attended ones only, cut to their host-side
        count (``eavqa_build_row_plan``; without ``lengths`` that count is one device->host read)."""
        if not pack:
            return RowPlan(cu=None, src=src, pos=pos, flat=None, row_labels=None, M=B * S, attn_mask=mask)
        cu, src_r, pos_r, row_labels, flat = ops.build_row_plan(mask, labels, src, pos, True)
        M = int(sum(lengths)) if lengths is not None else int(cu[-1].item())
        return RowPlan(cu=cu, src=src_r[:M], pos=pos_r[:M], flat=flat[:M], row_labels=row_labels[:M] if labels is not None else None, M=M,
                       attn_mask=None)

    def _norm(self, x: Tensor, g: Tensor, b: Optional[Tensor], save: bool, quantize: bool = True):
        """LayerNorm - without a ``b``: RMSNorm - of the stream -> ``(a, mean, rstd)``, the statistics None unless ``save`` (RMSNorm has
        no mean).  ``quantize`` (ln_1 / ln_2, in front of a Linear): with e4m3 weights and ``fuse_quantizer`` ``a`` is the row-quantised
        pair straight from the LayerNorm kernel (eavqa_layernorm_fwd_fp8: the bytes eavqa_quantize_rows_fp8 would produce, one pass less)."""
        if b is None:
            r = ops.rmsnorm_fwd(x, g, self.cfg.eps, self.dtype, save_stats=save)
            return (r[0], None, r[1]) if save else (r, None, None)
        if quantize and self.fp8 and self.fuse_quantizer:
            q, scale, *stats = ops.layernorm_fwd_fp8(x, g, b, self.cfg.eps, save_stats=save)
            return ((q, scale), *stats) if save else ((q, scale), None, None)
        r = ops.layernorm_fwd(x, g, b, self.cfg.eps, self.dtype, save_stats=save)
        return r if save else (r, None, None)

    def final_norm(self, x: Tensor) -> Tensor:
        """The model's final norm of the rows ``x`` (strided is fine) in the compute dtype, no statistics kept."""
        return self._norm(x, self.lnf_g, self.lnf_b, save=False, quantize=False)[0]

    def _ffn(self, L: _Layer, a2: Tensor, x1: Tensor, save: bool, hint: Callable, nxt):
        """Feed-forward of ``a2`` + residual ``x1`` -> (stream, ``u``): ``u`` is the activation's input, kept for act' when ``save`` - or
        (``gated``) the gate | up rows of the one GEMM, which SwiGLU folds.  ``nxt``: the weight the next GEMM of the pass streams."""
        c = self.cfg
        if self.gated:
            u = linear(a2, L.w_fc1, prefetch=hint(L.w_fc2))                                       # [M, 2F] = [gate x | up x]
            h = ops.swiglu_fwd(u)
        else:
            u = torch.empty((x1.shape[0], c.ffn), device=self.device, dtype=self.dtype) if save else None
            h = linear(a2, L.w_fc1, bias=L.b_fc1, act=c.act, aux_out=u, prefetch=hint(L.w_fc2))
        return linear(h, L.w_fc2, bias=L.b_fc2, residual=x1, out_f32=True, prefetch=hint(nxt)), u

    def layer_loop(self, x: Tensor, attend: Callable, save: bool, hints: bool, pos: Optional[Tensor] = None):
        """Every decoder layer over the fp32 stream ``x`` [M, E] -> (stream behind the last layer, [LayerTape] when ``save`` else None):
        norm, QKV, (``rotary``: q / k turned by ``pos``, int32, one entry per row), attention, out-projection + residual, norm,
        feed-forward + residual; a family without biases has None in their place.
        ``attend(li, q, k, v) -> (ctx, lse)`` is layer li's attention over column views of its QKV rows (``lse`` None unless the tape
        needs it).  ``hints``: every GEMM names the weight of the next one (:meth:`_hint`; the last names the lm_head)."""
        c, E = self.cfg, self.cfg.n_embd
        hint = self._hint if hints else _no_hint
        tape = [] if save else None
        for li, L in enumerate(self.layers):
            a, mean1, rstd1 = self._norm(x, L.ln1_g, L.ln1_b, save)
            qkv = linear(a, L.w_qkv, bias=L.b_qkv, prefetch=hint(L.w_o))
            if self.rotary:
                ops.rope(qkv, 2 * c.n_head, c.head_dim, pos, self.rope_cos, self.rope_sin)
            ctx, lse = attend(li, qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:])
            x1 = linear(ctx, L.w_o, bias=L.b_o, residual=x, out_f32=True, prefetch=hint(L.w_fc1))
            a2, mean2, rstd2 = self._norm(x1, L.ln2_g, L.ln2_b, save)
            nxt = self.layers[li + 1].w_qkv if li + 1 < len(self.layers) else self.head
            x2, u = self._ffn(L, a2, x1, save, hint, nxt)
            if save:
                tape.append(LayerTape(x, mean1, rstd1, qkv, ctx, lse, x1, mean2, rstd2, u))
            x = x2
        return x, tape

    def layer_loop_folded(self, x: Tensor, attend: Callable, save: bool):
        """:meth:`layer_loop` on the ``fold_layernorm`` route (eavqa_gemm_ln, no hints): only ln_1 of layer 0 is a kernel.  Every
        projection that writes the stream leaves it a second time in the compute dtype together with its row sums, and the LayerNorm
        behind it is a term of the next projection's epilogue, which also writes the statistics the tape keeps."""
        self._prepare_fold()
        c, T, E, M = self.cfg, self.dtype, self.cfg.n_embd, x.shape[0]
        f32 = dict(device=self.device, dtype=torch.float32)
        copy = lambda: (torch.empty((M, E), device=self.device, dtype=T), torch.empty((M, (E + 63) // 64, 2), **f32))
        stats = lambda: (torch.empty(M, **f32), torch.empty(M, **f32)) if save else (None, None)      # (mean, rstd) an epilogue writes
        tape = [] if save else None
        L0 = self.layers[0]
        a, mean1, rstd1 = self._norm(x, L0.ln1_g, L0.ln1_b, save)
        qkv = linear(a, L0.w_qkv, bias=L0.b_qkv)
        for li, L in enumerate(self.layers):
            ctx, lse = attend(li, qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:])
            x1T, st1 = copy()
            x1 = ops.gemm(ctx, L.w_o, bias=L.b_o, residual=x, out_f32=True, copy_out=x1T, stats_out=st1)
            mean2, rstd2 = stats()
            u = torch.empty((M, c.ffn), device=self.device, dtype=T) if save else None
            f = ops.gemm(x1T, L.w_fc1_f, bias=L.d_fc1, act=c.act, aux_out=u, ln_stats=st1, ln_c=L.c_fc1, ln_eps=c.eps, ln_save=(mean2, rstd2))
            below = self.layers[li + 1] if li + 1 < len(self.layers) else None
            xT, st = copy() if below is not None else (None, None)
            x2 = ops.gemm(f, L.w_fc2, bias=L.b_fc2, residual=x1, out_f32=True, copy_out=xT, stats_out=st)
            if save:
                tape.append(LayerTape(x, mean1, rstd1, qkv, ctx, lse, x1, mean2, rstd2, u))
            x = x2
            if below is not None:                             # ln_1 of the next layer: a term of its QKV projection
                mean1, rstd1 = stats()
                qkv = ops.gemm(xT, below.w_qkv_f, bias=below.d_qkv, ln_stats=st, ln_c=below.c_qkv, ln_eps=c.eps, ln_save=(mean1, rstd1))
        return x, tape

    def _head(self, hf: Tensor) -> Tensor:
        """lm_head GEMM into a [rows, vpad] fp32 buffer (pad columns are never read)."""
        lg = torch.empty((hf.shape[0], self.vpad), device=self.device, dtype=torch.float32)
        if self.head_q is not None:
            linear(hf, self.head_q, out=lg[:, :self.vocab])
            return lg
        if hf.shape[0] <= 64 and hf.dtype == torch.bfloat16 and self.vocab % 4 == 0 and self.cfg.n_embd % 32 == 0:
            # a decode step: stream the [V, E] head once with K split over workgroups (csrc/decode.hip)
            ops.splitk_finish(ops.gemm_splitk(hf, self.head[:self.vocab]), [lg[:, :self.vocab]])
        else:
            ops.gemm(hf, self.head, out=lg[:, :self.vocab])
        return lg

    # ---------------------------------------------------------------- backward (dgrad only)
    def backward(self, tape: Tape, gloss: Tensor, n_prefix_rows: int) -> Tensor:
        """d loss / d prefix_rows.  ``gloss``: float32 [1] upstream gradient of the scalar loss."""
        self._prepare_backward()
        c, T = self.cfg, self.dtype
        E, H, hd = c.n_embd, c.n_head, c.head_dim
        B, S, M = tape.B, tape.S, tape.M
        scale = hd ** -0.5
        lowp = T != torch.float32

        # the residual-stream gradient lives in fp32 (dx); each norm backward also emits the copy in the
        # compute dtype that the next dgrad GEMM consumes as its A operand (no separate cast pass)
        dlog = ops.ce_bwd(tape.logits, tape.labels, self.vocab, tape.row_lse, tape.count, gloss, T, self.vpad)
        hint = self._hint                                                 # the next GEMM's weight (eavqa_gemm_pf), as in forward
        dhf = linear(dlog, self.head_t, prefetch=hint(self.layers[-1].w_fc2_t))   # [M,E] (or [n_scored,E])
        if tape.sel is not None:
            dhf = ops.scatter_rows(dhf, tape.sel, M)                         # rows without a label get no gradient here
        # the copy of the stream gradient that the next dgrad GEMM multiplies (dxT) leaves the norm backward in the compute dtype - or,
        # with e4m3 weights and ``fuse_quantizer``, already row-quantised
        fused, rms = self.fp8 and self.fuse_quantizer, self.lnf_b is None
        if fused:
            dxT = (torch.empty((M, E), device=self.device, dtype=torch.uint8), torch.empty(M, device=self.device, dtype=torch.float32))
        else:
            dxT = torch.empty((M, E), device=self.device, dtype=T) if lowp else None

        def norm_bwd(xx, dy, g, mean, rstd, **kw):
            if fused:
                return ops.layernorm_bwd_fp8(xx, dy, g, mean, rstd, dxT[0], dxT[1], **kw)
            if rms:
                return ops.rmsnorm_bwd(xx, dy, g, rstd, lowp_out=dxT, **kw)
            return ops.layernorm_bwd(xx, dy, g, mean, rstd, lowp_out=dxT, **kw)

        dx = norm_bwd(tape.x_last, dhf, self.lnf_g, tape.meanf, tape.rstdf)
        for li, (L, t) in enumerate(zip(reversed(self.layers), reversed(tape.layers))):
            da2 = self._ffn_bwd(L, dxT if lowp else dx, t.u, hint)           # [M,E]
            dx1 = norm_bwd(t.x1, da2, L.ln2_g, t.mean2, t.rstd2, dres=dx, out=dx)
            dctx = linear(dxT if lowp else dx1, L.w_o_t, prefetch=hint(L.w_qkv_t))   # [M,E]
            dqkv = torch.empty_like(t.qkv)
            q, k, v = t.qkv[:, :E], t.qkv[:, E:2 * E], t.qkv[:, 2 * E:]
            ops.attention_bwd(q, k, v, t.ctx, dctx, t.lse, B, H, S, S, hd, key_mask=tape.mask, causal=True, scale=scale,
                              dq=dqkv[:, :E], dk=dqkv[:, E:2 * E], dv=dqkv[:, 2 * E:], cu_seqlens=tape.cu)
            if self.rotary:                                               # the rotation is orthogonal: its transpose is its backward
                ops.rope(dqkv, 2 * H, hd, tape.pos, self.rope_cos, self.rope_sin, inverse=True)
            below = self.layers[len(self.layers) - 2 - li].w_fc2_t if li + 1 < len(self.layers) else None
            da = linear(dqkv, L.w_qkv_t, prefetch=hint(below))            # [M,E]
            dx = norm_bwd(t.x, da, L.ln1_g, t.mean1, t.rstd1, dres=dx1, out=dx1)
        return ops.embed_assemble_bwd(tape.src, dx, n_prefix_rows, T)

    def _ffn_bwd(self, L: _Layer, dx: Tensor, u: Tensor, hint: Callable) -> Tensor:
        """d loss / d (the feed-forward's input) [M, E] from the stream gradient ``dx`` in the dgrad GEMM's operand form."""
        if self.gated:
            dh = linear(dx, L.w_fc2_t, prefetch=hint(L.w_fc1_t))             # [M,F]
            du = ops.swiglu_bwd(u, dh)                                       # [M,2F] = d gate | d up
        else:
            du = linear(dx, L.w_fc2_t, act=self.cfg.act, aux_in=u, prefetch=hint(L.w_fc1_t))   # (dx W2) * act'(u)   [M,F]
        return linear(du, L.w_fc1_t, prefetch=hint(L.w_o_t))


def _same(a: Tensor, b: Tensor) -> bool:
    try:
        return a.data_ptr() == b.data_ptr() or bool(torch.equal(a.to(b.device, b.dtype), b))
    except Exception:
        return False
