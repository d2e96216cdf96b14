"""Tensor-level wrappers over the C ABI (include/eavqa.h).

PyTorch supplies device memory and the current HIP stream; every arithmetic op on the hot path
is one of the calls below.  Nothing here computes with torch ops on the data path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib, _lib_llama
from ._lib import ACT, BF16, F32, call

Tensor = torch.Tensor


F16 = _lib.EAVQA_F16   # storage type of a frozen tower's residual stream only (layernorm_fwd x / y, gemm residual / out)
_X_KIND = {torch.float32: 1, torch.bfloat16: 2, torch.float16: 3}   # input kind of the norm kernels (their `x_kind` argument)


def dtype_id(dt: torch.dtype, stream: bool = False) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if stream and dt == torch.float16:
        return F16
    raise _lib.EavqaError(f"unsupported storage dtype {dt}")


def _stream() -> int:
    # raw HIP stream handle of torch's current stream (the fast private accessor: the public
    # torch.cuda.current_stream() costs several microseconds per call, which adds up over ~1300 launches a step)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


class KernelSelect:
    """Kernel selectors handed to the ``*_ex`` entry points of include/eavqa_test.h.  Both are 0 in the product path (the
    library chooses by shape); the parity tests and tools/gemm_bench.py set them to cover / time a particular kernel.  The
    state lives HERE, in the test-facing Python layer - libeavqa_hip.so itself holds no mutable state."""
    gemm = 0
    attention = 0


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev(t: Tensor) -> None:
    if not t.is_cuda:
        raise _lib.EavqaError("eavqa ops run on the GPU only (no CPU fallback): got a CPU tensor")


def _ld(t: Tensor) -> int:
    """Leading dimension of a 2-D (or flattened row-major) tensor whose last dim is contiguous."""
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        raise _lib.EavqaError("last dimension must be contiguous")
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


def gemm(a: Tensor, b: Tensor, *, a_kc: bool = True, b_kc: bool = True, bias: Optional[Tensor] = None,
         act: str = "none", aux_in: Optional[Tensor] = None, aux_out: Optional[Tensor] = None,
         residual: Optional[Tensor] = None, out: Optional[Tensor] = None, out_f32: bool = False,
         alpha: float = 1.0, copy_out: Optional[Tensor] = None, stats_out: Optional[Tensor] = None, ln_stats: Optional[Tensor] = None,
         ln_c: Optional[Tensor] = None, ln_eps: float = 1e-5, ln_save: Optional[Tuple[Tensor, Tensor]] = None,
         prefetch: Optional[Tensor] = None) -> Tensor:
    """``C = epilogue(alpha * A @ B^T)`` - see eavqa_gemm.  ``a``: [M,K] (a_kc) or [K,M];
    ``b``: [N,K] (b_kc, nn.Linear layout) or [K,N] (Conv1D layout).

    eavqa_gemm_ln (a frozen pre-LN layer's LayerNorm folded into its neighbours), producer side: ``copy_out`` [M, N] in the operand
    dtype, ``stats_out`` float32 [M, >= ceil(N / 64), 2]; consumer side: ``ln_stats`` (a producer's ``stats_out`` for the rows of
    ``a``), ``ln_c`` float32 [N], ``ln_eps``, ``ln_save`` = (mean, rstd) float32 [M] to be written.

    ``prefetch`` (eavqa_gemm_pf): the contiguous weight tensor the NEXT GEMM in program order will stream; the kernel touches its lines so that it
    waits in the Infinity Cache.  Only read; the result is bit-for-bit the same.  Not combined with the eavqa_gemm_ln arguments or a kernel selector."""
    _dev(a)
    M, K = (a.shape if a_kc else (a.shape[1], a.shape[0]))
    N, Kb = (b.shape if b_kc else (b.shape[1], b.shape[0]))
    if K != Kb:
        raise _lib.EavqaError(f"gemm inner dims differ: {K} vs {Kb}")
    if a.dtype != b.dtype:
        raise _lib.EavqaError("gemm operands must share a dtype")
    dt = dtype_id(a.dtype)
    half = torch.float16                                    # 16-bit stream of a frozen tower (bf16 operands): EAVQA_GEMM_STREAM_F16
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    elif out.dtype != torch.float32 and out.dtype != a.dtype and not (out.dtype == half and a.dtype == torch.bfloat16):
        raise _lib.EavqaError("gemm out dtype must be float32, the operand dtype or (bf16 operands) float16")
    out_f32 = out.dtype == torch.float32
    aux = aux_in if aux_in is not None else aux_out
    flags = _lib.EAVQA_GEMM_OUT_F32 if out_f32 else 0
    if residual is not None and residual.dtype != torch.float32:
        if residual.dtype != a.dtype and not (residual.dtype == half and a.dtype == torch.bfloat16):
            raise _lib.EavqaError("gemm residual must be float32, the operand dtype or (bf16 operands) float16")
        flags |= _lib.EAVQA_GEMM_RESIDUAL_LOWP              # the residual stream of a frozen tower in 16 bits
    stream_half = (out.dtype == half) or (residual is not None and residual.dtype == half)
    if stream_half:
        if (out.dtype not in (half, torch.float32)) or (residual is not None and residual.dtype not in (half, torch.float32)):
            raise _lib.EavqaError("gemm: a float16 stream needs float16 (or float32) for both the residual and the output")
        flags |= _lib.EAVQA_GEMM_STREAM_F16
    args = (dt, int(a_kc), int(b_kc), M, N, K, _p(a), _ld(a), _p(b), _ld(b), _p(out), _ld(out),
            flags, float(alpha), _p(bias), ACT[act], _p(aux_in), _p(aux_out), _ld(aux) if aux is not None else 0,
            _p(residual), _ld(residual) if residual is not None else 0, _stream())
    ln_form = copy_out is not None or stats_out is not None or ln_stats is not None
    if prefetch is not None:
        if not prefetch.is_contiguous() or prefetch.device != a.device:
            raise _lib.EavqaError("gemm prefetch must be a contiguous tensor on the operands' device")
        if ln_form or KernelSelect.gemm:
            raise _lib.EavqaError("gemm prefetch cannot be combined with the eavqa_gemm_ln arguments or a kernel selector")
        call("eavqa_gemm_pf", *args, prefetch.data_ptr(), prefetch.numel() * prefetch.element_size())
    elif ln_form:
        g = _lib.GemmLn()
        if copy_out is not None:
            if copy_out.dtype != a.dtype or tuple(copy_out.shape) != (M, N):
                raise _lib.EavqaError("gemm copy_out must be [M, N] in the operand dtype")
            g.copy_out, g.ld_copy = _p(copy_out), _ld(copy_out)
        if stats_out is not None:
            if stats_out.dtype != torch.float32 or stats_out.dim() != 3 or stats_out.shape[0] != M or stats_out.shape[2] != 2 or not stats_out.is_contiguous():
                raise _lib.EavqaError("gemm stats_out must be a contiguous float32 [M, slots, 2]")
            g.stats_out, g.stats_ld = _p(stats_out), stats_out.shape[1]
        if ln_stats is not None:
            if ln_stats.dtype != torch.float32 or ln_stats.dim() != 3 or ln_stats.shape[0] != M or ln_stats.shape[2] != 2 or not ln_stats.is_contiguous():
                raise _lib.EavqaError("gemm ln_stats must be a contiguous float32 [M, slots, 2]")
            if ln_c is None or ln_c.dtype != torch.float32 or ln_c.numel() != N:
                raise _lib.EavqaError("gemm ln_c must be float32 [N]")
            g.ln_stats, g.ln_parts, g.ln_ld, g.ln_cols = _p(ln_stats), ln_stats.shape[1], ln_stats.shape[1], K
            g.ln_c, g.ln_eps = _p(ln_c), float(ln_eps)
            if ln_save is not None:
                g.mean_out, g.rstd_out = _p(ln_save[0]), _p(ln_save[1])
        if KernelSelect.gemm:
            call("eavqa_gemm_ln_ex", *args[:-1], C.byref(g), args[-1], KernelSelect.gemm)
        else:
            call("eavqa_gemm_ln", *args[:-1], C.byref(g), args[-1])
    elif KernelSelect.gemm:
        call("eavqa_gemm_ex", *args, KernelSelect.gemm)
    else:
        call("eavqa_gemm", *args)
    return out


def quantize_rows_fp8(x: Tensor, out: Optional[Tensor] = None, scale_out: Optional[Tensor] = None):
    """Rows of ``x`` (bf16 / fp32 [rows, cols]) -> (e4m3 bytes as uint8 [rows, cols], float32 row scales [rows]).  ``out`` / ``scale_out``:
    views to write them to (a uint8 [rows, cols] view whose last dimension is contiguous, a float32 [rows] view of unit stride)."""
    _dev(x)
    rows, cols = x.shape
    q = torch.empty((rows, cols), device=x.device, dtype=torch.uint8) if out is None else out
    sc = torch.empty(rows, device=x.device, dtype=torch.float32) if scale_out is None else scale_out
    if q.dtype != torch.uint8 or tuple(q.shape) != (rows, cols) or q.device != x.device:
        raise _lib.EavqaError("quantize_rows_fp8 out must be a uint8 [rows, cols] view on the input's device")
    if sc.dtype != torch.float32 or tuple(sc.shape) != (rows,) or sc.device != x.device or (rows > 1 and sc.stride(0) != 1):
        raise _lib.EavqaError("quantize_rows_fp8 scale_out must be a float32 [rows] view of unit stride on the input's device")
    call("eavqa_quantize_rows_fp8", dtype_id(x.dtype), rows, cols, _p(x), _ld(x), _p(q), _ld(q), _p(sc), _stream())
    return q, sc


def gemm_fp8(a_q: Tensor, a_scale: Tensor, b_q: Tensor, b_scale: float, *, bias: Optional[Tensor] = None, act: str = "none",
             aux_in: Optional[Tensor] = None, aux_out: Optional[Tensor] = None, residual: Optional[Tensor] = None,
             out: Optional[Tensor] = None, out_f32: bool = False, alpha: float = 1.0, tile: int = 0) -> Tensor:
    """``C = epilogue(alpha * b_scale * a_scale[m] * A_q @ B_q^T)`` on e4m3 operands (uint8 storage) - see eavqa_gemm_fp8.
    Outputs / aux are bfloat16 (or float32 ``out``)."""
    _dev(a_q)
    M, K = a_q.shape
    N = b_q.shape[0]
    if b_q.shape[1] != K:
        raise _lib.EavqaError(f"gemm_fp8 inner dims differ: {K} vs {b_q.shape[1]}")
    if out is None:
        out = torch.empty((M, N), device=a_q.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    aux = aux_in if aux_in is not None else aux_out
    call("eavqa_gemm_fp8", M, N, K, _p(a_q), _ld(a_q), _p(a_scale), _p(b_q), _ld(b_q), float(b_scale), _p(out), _ld(out),
         int(out.dtype == torch.float32), float(alpha), _p(bias), ACT[act], _p(aux_in), _p(aux_out), _ld(aux) if aux is not None else 0,
         _p(residual), _ld(residual) if residual is not None else 0, _stream(), int(tile))
    return out


def layernorm_fwd(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float, out_dtype: torch.dtype,
                  save_stats: bool = False, out: Optional[Tensor] = None):
    """Rows of ``x`` ([rows, cols]: float32, bfloat16 or float16) -> ``y`` in ``out_dtype`` (+ mean, rstd).  float16 is the storage
    type of a frozen tower's residual stream only (models/clip_vit.py)."""
    _dev(x)
    rows, cols = x.shape
    y = out if out is not None else torch.empty((rows, cols), device=x.device, dtype=out_dtype)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    x_kind = _X_KIND.get(x.dtype)
    if x_kind is None:
        raise _lib.EavqaError(f"unsupported layernorm input dtype {x.dtype}")
    call("eavqa_layernorm_fwd", dtype_id(out_dtype, stream=True), x_kind, rows, cols, _p(x), _ld(x),
         _p(gamma), _p(beta), float(eps), _p(y), _ld(y), _p(mean), _p(rstd), _stream())
    return (y, mean, rstd) if save_stats else y


def layernorm_fwd_fp8(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float, save_stats: bool = False):
    """LayerNorm whose bf16 result leaves as e4m3 rows + row scales (``layernorm_fwd`` followed by ``quantize_rows_fp8``, one kernel):
    ``(q uint8 [rows, cols], scale float32 [rows])`` (+ mean, rstd)."""
    _dev(x)
    rows, cols = x.shape
    q = torch.empty((rows, cols), device=x.device, dtype=torch.uint8)
    sc = torch.empty(rows, device=x.device, dtype=torch.float32)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    x_kind = _X_KIND.get(x.dtype)
    if x_kind is None:
        raise _lib.EavqaError(f"unsupported layernorm input dtype {x.dtype}")
    call("eavqa_layernorm_fwd_fp8", x_kind, rows, cols, _p(x), _ld(x), _p(gamma), _p(beta), float(eps), _p(q), _ld(q), _p(sc), _p(mean), _p(rstd),
         _stream())
    return (q, sc, mean, rstd) if save_stats else (q, sc)


def layernorm_bwd_fp8(x: Tensor, dy: Tensor, gamma: Optional[Tensor], mean: Tensor, rstd: Tensor, q_out: Tensor, scale_out: Tensor,
                      dres: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``layernorm_bwd`` whose bf16 copy of dx leaves as e4m3 rows + row scales into ``q_out`` (uint8 [rows, cols]) / ``scale_out``."""
    _dev(x)
    rows, cols = x.shape
    if dy.dtype != torch.bfloat16:
        raise _lib.EavqaError("layernorm_bwd_fp8: dy must be bfloat16")
    dx = out if out is not None else torch.empty((rows, cols), device=x.device, dtype=torch.float32)
    if dres is not None and _ld(dres) != _ld(dx):
        raise _lib.EavqaError("dres must share dx's leading dimension")
    call("eavqa_layernorm_bwd_fp8", int(x.dtype == torch.float32), rows, cols, _p(x), _ld(x), _p(dy), _ld(dy), _p(gamma), _p(mean), _p(rstd),
         _p(dres), _p(dx), _ld(dx), _p(q_out), _ld(q_out), _p(scale_out), _stream())
    return dx


def layernorm_bwd(x: Tensor, dy: Tensor, gamma: Optional[Tensor], mean: Tensor, rstd: Tensor,
                  dres: Optional[Tensor] = None, dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None,
                  out: Optional[Tensor] = None, lowp_out: Optional[Tensor] = None) -> Tensor:
    """``lowp_out``: optional [rows, cols] tensor in ``dy.dtype`` that receives a second copy of dx."""
    _dev(x)
    rows, cols = x.shape
    dx = out if out is not None else torch.empty((rows, cols), device=x.device, dtype=torch.float32)
    if dres is not None and _ld(dres) != _ld(dx):
        raise _lib.EavqaError("dres must share dx's leading dimension")
    call("eavqa_layernorm_bwd", dtype_id(dy.dtype), int(x.dtype == torch.float32), rows, cols, _p(x), _ld(x), _p(dy), _ld(dy),
         _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), _ld(dx), _p(dgamma), _p(dbeta), _p(lowp_out),
         _ld(lowp_out) if lowp_out is not None else 0, _stream())
    return dx


def attention_fwd(q: Tensor, k: Tensor, v: Tensor, B: int, H: int, Sq: int, Sk: int, hd: int, *,
                  key_mask: Optional[Tensor] = None, causal: bool = False, scale: float = 1.0, save_lse: bool = False,
                  q_batch_rows: int = 0, kv_batch_rows: int = 0, ld_mask: int = 0, out: Optional[Tensor] = None,
                  cu_seqlens: Optional[Tensor] = None):
    """``q``: rows [B*Sq, >=H*hd] views (element (b,s,h,d) at row b*Sq+s, col h*hd+d); same for k/v.
    With ``cu_seqlens`` the rows are packed (sample b = rows cu[b]..cu[b+1]) and ``Sq`` is the longest sample."""
    _dev(q)
    o = out if out is not None else torch.empty((q.shape[0] if cu_seqlens is not None else B * Sq, H * hd), device=q.device, dtype=q.dtype)
    lse = torch.empty((B, H, Sq), device=q.device, dtype=torch.float32) if save_lse else None
    if B * H > ATTN_MAX_PAIRS and cu_seqlens is None:
        launches = _attn_batches(B, H, Sq, Sk, q, k, v, o, key_mask, lse, q_batch_rows, kv_batch_rows, ld_mask)
    else:
        launches = ((B, _p(q), _p(k), _p(v), _p(o), _p(key_mask), _p(lse)),)
    for n, pq, pk, pv, po, pm, pl in launches:
        args = (dtype_id(q.dtype), n, H, Sq, Sk, hd, pq, _ld(q), pk, _ld(k), pv, _ld(v), po, _ld(o),
                q_batch_rows, kv_batch_rows, pm, ld_mask, _p(cu_seqlens), int(causal), float(scale), pl, _stream())
        if KernelSelect.attention:
            call("eavqa_attention_fwd_ex", *args, KernelSelect.attention)
        else:
            call("eavqa_attention_fwd", *args)
    return (o, lse) if save_lse else o


ATTN_MAX_PAIRS = 65535      # (sample, head) pairs one attention launch takes (the second grid dimension)


def _attn_batches(B, H, Sq, Sk, q, k, v, o, key_mask, lse, q_batch_rows, kv_batch_rows, ld_mask):
    """A batched attention forward whose B * H exceeds the grid (answer scoring: questions x candidates) as several launches over
    consecutive samples - the same arithmetic per sample: ``[(samples, q, k, v, o, key_mask, lse pointers), ...]``."""
    step = max(1, ATTN_MAX_PAIRS // H)
    qb, kb, mb = (q_batch_rows or Sq), (kv_batch_rows or Sk), (ld_mask or Sk)
    at = lambda t, rows: t.data_ptr() + rows * _ld(t) * t.element_size()
    return [(min(step, B - b0), at(q, b0 * qb), at(k, b0 * kb), at(v, b0 * kb), at(o, b0 * qb),
             None if key_mask is None else key_mask.data_ptr() + b0 * mb * 4, None if lse is None else lse.data_ptr() + b0 * H * Sq * 4)
            for b0 in range(0, B, step)]


def attention_decode(q: Tensor, k_cache: Tensor, v_cache: Tensor, k_new: Tensor, v_new: Tensor, B: int, H: int, Sk: int, hd: int, *,
                     kv_batch_rows: int, key_mask: Optional[Tensor] = None, ld_mask: int = 0, scale: float = 1.0,
                     out: Optional[Tensor] = None) -> Tensor:
    """One decode step that appends: ``k_new`` / ``v_new`` (row views [B, H*hd]) go to position ``Sk - 1`` of every sample's cache
    (``k_cache`` / ``v_cache`` row views [B*kv_batch_rows, H*hd]) and ``q`` [B, H*hd] attends over positions ``0 .. Sk-1``."""
    _dev(q)
    o = out if out is not None else torch.empty((B, H * hd), device=q.device, dtype=q.dtype)
    call("eavqa_attention_decode", dtype_id(q.dtype), B, H, Sk, hd, _p(q), _ld(q), _p(k_cache), _ld(k_cache), _p(v_cache), _ld(v_cache),
         kv_batch_rows, _p(k_new), _p(v_new), _ld(k_new), _p(o), _ld(o), _p(key_mask), ld_mask, float(scale), _stream())
    return o


def attention_decode_shared(q: Tensor, k_prompt: Tensor, v_prompt: Tensor, k_tail: Tensor, v_tail: Tensor, k_new: Tensor, v_new: Tensor,
                            B: int, G: int, H: int, S0: int, t: int, hd: int, *, prompt_batch_rows: int, key_mask: Optional[Tensor] = None,
                            ld_mask: int = 0, scale: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """``eavqa_attention_decode_shared``: one decode step of B prompts x G rows (ordered (b, g)).  ``q`` / ``k_new`` / ``v_new``: row views
    [B*G, H*hd]; ``k_prompt`` / ``v_prompt``: row views [B*prompt_batch_rows, H*hd], shared by the G rows of a prompt and masked by
    ``key_mask`` int32 [B, >= S0]; ``k_tail`` / ``v_tail``: contiguous [B*G, t_max, H*hd], positions 0..t-1 attended, position ``t``
    appended from ``k_new`` / ``v_new`` and attended."""
    _dev(q)
    if k_tail.dim() != 3 or k_tail.shape != v_tail.shape or k_tail.shape[0] != B * G or not (k_tail.is_contiguous() and v_tail.is_contiguous()):
        raise _lib.EavqaError("attention_decode_shared: contiguous tails [B*G, t_max, H*hd]")
    if len({q.dtype, k_prompt.dtype, v_prompt.dtype, k_tail.dtype, k_new.dtype, v_new.dtype}) != 1:
        raise _lib.EavqaError("attention_decode_shared: one storage dtype")
    o = out if out is not None else torch.empty((B * G, H * hd), device=q.device, dtype=q.dtype)
    call("eavqa_attention_decode_shared", dtype_id(q.dtype), B, G, H, S0, int(t), k_tail.shape[1], hd, _p(q), _ld(q), _p(k_prompt), _ld(k_prompt),
         _p(v_prompt), _ld(v_prompt), prompt_batch_rows, _p(k_tail), _p(v_tail), k_tail.shape[2], _p(k_new), _p(v_new), _ld(k_new), _p(o), _ld(o),
         _p(key_mask), ld_mask, float(scale), _stream())
    return o


def attention_decode_splitk(part: Tensor, bias: Optional[Tensor], k_cache: Tensor, v_cache: Tensor, B: int, H: int, Sk: int, hd: int, *,
                            kv_batch_rows: int, key_mask: Optional[Tensor] = None, ld_mask: int = 0, scale: float = 1.0,
                            out: Optional[Tensor] = None) -> Tensor:
    """``attention_decode`` straight from the QKV projection's split-K partial sums ``part`` [ks, B, 3*H*hd] (+ ``bias`` [3*H*hd])."""
    _dev(part)
    o = out if out is not None else torch.empty((B, H * hd), device=part.device, dtype=k_cache.dtype)
    call("eavqa_attention_decode_splitk", dtype_id(k_cache.dtype), B, H, Sk, hd, _p(part), part.shape[0], _p(bias), _p(k_cache), _ld(k_cache),
         _p(v_cache), _ld(v_cache), kv_batch_rows, _p(o), _ld(o), _p(key_mask), ld_mask, float(scale), _stream())
    return o


def attention_bwd(q, k, v, o, d_o, lse, B, H, Sq, Sk, hd, *, key_mask=None, causal=False, scale=1.0,
                  dq=None, dk=None, dv=None, cu_seqlens=None):
    _dev(q)
    nq = q.shape[0] if cu_seqlens is not None else B * Sq
    nk = k.shape[0] if cu_seqlens is not None else B * Sk
    dq = dq if dq is not None else torch.empty((nq, H * hd), device=q.device, dtype=q.dtype)
    dk = dk if dk is not None else torch.empty((nk, H * hd), device=q.device, dtype=q.dtype)
    dv = dv if dv is not None else torch.empty((nk, H * hd), device=q.device, dtype=q.dtype)
    delta = torch.empty((B, H, Sq), device=q.device, dtype=torch.float32)
    args = (dtype_id(q.dtype), B, H, Sq, Sk, hd, _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(o), _ld(o),
            _p(d_o), _ld(d_o), _p(dq), _ld(dq), _p(dk), _ld(dk), _p(dv), _ld(dv), _p(key_mask), _p(cu_seqlens), int(causal),
            float(scale), _p(lse), _p(delta), _stream())
    if KernelSelect.attention:
        call("eavqa_attention_bwd_ex", *args, KernelSelect.attention)
    else:
        call("eavqa_attention_bwd", *args)
    return dq, dk, dv


def build_prefix_rows(tokens: Tensor, question_mask: Tensor, L: int, pos_mode: int, prefix_row_stride: Optional[int] = None,
                      prefix_row_offset: int = 0):
    """int64 [B,T] tokens/mask -> (src, mask, pos) int32 [B, L+T]."""
    _dev(tokens)
    B, T = tokens.shape
    tokens = tokens.contiguous()
    qm = question_mask.to(torch.int64).contiguous()
    S = L + T
    src = torch.empty((B, S), device=tokens.device, dtype=torch.int32)
    msk = torch.empty_like(src)
    pos = torch.empty_like(src)
    call("eavqa_build_prefix_rows", B, L, T, _p(tokens), _p(qm), pos_mode, L if prefix_row_stride is None else prefix_row_stride,
         prefix_row_offset, _p(src), _p(msk), _p(pos), _stream())
    return src, msk, pos


def build_fewshot_rows(tokens: Tensor, question_mask: Tensor, L: int, n_img: int, special_token_id: int, pos_mode: int):
    _dev(tokens)
    B, T = tokens.shape
    tokens = tokens.contiguous()
    qm = question_mask.to(torch.int64).contiguous()
    T_out = T + (L - 1) * n_img
    src = torch.empty((B, T_out), device=tokens.device, dtype=torch.int32)
    msk = torch.empty_like(src)
    pos = torch.empty_like(src)
    status = torch.empty(B, device=tokens.device, dtype=torch.int32)
    call("eavqa_build_fewshot_rows", B, T, L, n_img, int(special_token_id), _p(tokens), _p(qm), pos_mode, _p(src), _p(msk),
         _p(pos), _p(status), _stream())
    return src, msk, pos, status


def build_fewshot_labels(tokens: Tensor, labels: Tensor, L: int, n_img: int, special_token_id: int):
    """int64 [B,T] tokens/labels -> (labels_out int64 [B, T+(L-1)*n_img], scored int32 [B]): ``labels`` through the interleave of
    :func:`build_fewshot_rows` (src/models/vct0.py:494-533), -100 on every prefix slot (clipcap.py:323-335) - also where ``labels``
    holds something on a sentinel - and on the tail of a row with too few sentinels; ``scored[b]`` counts the labels != -100 written.
    The layout comes from ``eavqa_build_fewshot_rows`` itself, so a label and its token cannot disagree on their position: every text
    token is replaced by a number that names its own column (above the sentinel range, so the walk sees the same sentinels), the kernel
    places those numbers, and the labels are gathered through them."""
    _dev(tokens)
    B, T = tokens.shape
    if tuple(labels.shape) != (B, T):
        raise ValueError(f"labels must be [B, T] = {(B, T)} like tokens, got {tuple(labels.shape)}")
    base = int(special_token_id) + 1
    if base <= 0 or base + T >= 2 ** 31:
        raise ValueError("special_token_id must be >= 0 and special_token_id + T fit the int32 rows of build_fewshot_rows")
    sentinel = (tokens <= special_token_id) & (tokens > special_token_id - n_img)
    column = torch.arange(base, base + T, device=tokens.device, dtype=torch.int64)
    src, _, _, _ = build_fewshot_rows(torch.where(sentinel, tokens, column), torch.ones_like(tokens), L, n_img, special_token_id, 0)
    col = src.to(torch.int64) - base                            # >= 0: a text position; prefix slots and the undefined tail are below
    out = torch.where(col >= 0, labels.to(torch.int64).gather(1, col.clamp(min=0)), torch.full_like(col, -100))
    return out, (out != -100).sum(1, dtype=torch.int32)


def embed_assemble(src: Tensor, pos: Optional[Tensor], wte: Tensor, prefix_rows: Optional[Tensor], wpe: Optional[Tensor],
                   out: Optional[Tensor] = None) -> Tensor:
    _dev(src)
    rows = src.numel()
    E = wte.shape[1]
    x = out if out is not None else torch.empty((rows, E), device=src.device, dtype=torch.float32)
    call("eavqa_embed_assemble", dtype_id(wte.dtype), rows, E, _p(src), _p(pos), _p(wte), _ld(wte), _p(prefix_rows),
         _ld(prefix_rows) if prefix_rows is not None else 0, _p(wpe), _ld(wpe) if wpe is not None else 0, _p(x), _ld(x), _stream())
    return x


def embed_assemble_bwd(src: Tensor, dx: Tensor, n_prefix_rows: int, dtype: torch.dtype) -> Tensor:
    rows, E = dx.shape
    d = torch.zeros((n_prefix_rows, E), device=dx.device, dtype=dtype)
    call("eavqa_embed_assemble_bwd", dtype_id(dtype), rows, E, _p(src), _p(dx), _ld(dx), _p(d), _ld(d), _stream())
    return d


def build_labels(input_ids: Tensor, L: int, pad_token_id: int, bos_token_id: int = -1, mode: int = 0) -> Tensor:
    _dev(input_ids)
    B, T = input_ids.shape
    ids = input_ids.contiguous()
    out = torch.empty((B, L + T), device=ids.device, dtype=torch.int64)
    call("eavqa_build_labels", mode, B, T, L, _p(ids), int(pad_token_id), int(bos_token_id), _p(out), _stream())
    return out


def build_row_plan(mask: Tensor, labels: Optional[Tensor], src: Tensor, pos: Tensor, pack: bool):
    """-> (cu_seqlens [B+1], src_rows, pos_rows, row_labels, flat_index), the row buffers sized B*S (first
    ``cu_seqlens[-1]`` entries valid)."""
    _dev(mask)
    B, S = mask.shape
    dev = mask.device
    cu = torch.empty(B + 1, device=dev, dtype=torch.int32)
    src_r = torch.empty(B * S, device=dev, dtype=torch.int32)
    pos_r = torch.empty(B * S, device=dev, dtype=torch.int32)
    flat = torch.empty(B * S, device=dev, dtype=torch.int32)
    lab = torch.empty(B * S, device=dev, dtype=torch.int64)
    call("eavqa_build_row_plan", B, S, int(pack), _p(mask), _p(labels), _p(src), _p(pos), _p(cu), _p(src_r), _p(pos_r), _p(lab),
         _p(flat), _stream())
    return cu, src_r, pos_r, lab, flat


def _ce_dims(labels: Tensor):
    """(B, S, rows): 2-D labels = unshifted [B,S]; 1-D labels = one shifted label per row (S = 0)."""
    if labels.dim() == 2:
        return labels.shape[0], labels.shape[1], labels.shape[0] * labels.shape[1]
    return labels.shape[0], 0, labels.shape[0]


def ce_fwd(logits: Tensor, labels: Tensor, V: int):
    """logits float32 [rows, ld>=V]; labels int64 [B,S] unshifted or [rows] shifted -> (loss[1], count[1], row_lse)."""
    _dev(logits)
    B, S, rows = _ce_dims(labels)
    row_loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    row_lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    count = torch.empty(1, device=logits.device, dtype=torch.float32)
    call("eavqa_ce_fwd", B, S, V, _p(logits), _ld(logits), _p(labels), _p(row_loss), _p(row_lse), _p(loss), _p(count), _stream())
    return loss, count, row_lse


def guard_count(count: Tensor, capacity: int, loss: Tensor) -> None:
    """``loss[0] = NaN`` on the device when ``count[0] > capacity`` (an under-sized scored-row compaction)."""
    call("eavqa_guard_count", _p(count), int(capacity), _p(loss), _stream())


def ce_bwd(logits: Tensor, labels: Tensor, V: int, row_lse: Tensor, count: Tensor, gscale: Tensor, dtype: torch.dtype,
           ldd: int) -> Tensor:
    B, S, rows = _ce_dims(labels)
    d = torch.empty((rows, ldd), device=logits.device, dtype=dtype)
    call("eavqa_ce_bwd", dtype_id(dtype), B, S, V, _p(logits), _ld(logits), _p(labels), _p(row_lse), _p(count), _p(gscale),
         _p(d), ldd, _stream())
    return d


def greedy_pick(logits: Tensor, V: int, pad_token_id: int, eos_token_id: Optional[int], raw: Tensor, emitted_col: Tensor,
                unfinished: Tensor, logprob: Optional[Tensor] = None, any_unfinished: Optional[Tensor] = None) -> None:
    """``emitted_col``: int64 view [B] of column t of the [B, max_length] token matrix; ``logprob``: float32 [B] or None;
    ``any_unfinished``: a ZEROED int32 element that reads 1 afterwards when some row is still unfinished (the early-stop flag)."""
    B = logits.shape[0]
    call("eavqa_greedy_pick", B, V, _p(logits), _ld(logits), int(pad_token_id if pad_token_id is not None else 0),
         int(eos_token_id) if eos_token_id is not None else -1, _p(raw), _p(emitted_col), emitted_col.stride(0),
         _p(unfinished), _p(logprob), _p(any_unfinished), _stream())


def sample_pick(logits: Tensor, V: int, temperature: float, top_k: int, top_p: float, seed: int, step: int, pad_token_id: int,
                eos_token_id: Optional[int], raw: Tensor, emitted_col: Tensor, unfinished: Optional[Tensor], logprob: Optional[Tensor] = None,
                any_unfinished: Optional[Tensor] = None, scores_out: Optional[Tensor] = None, uniform_in: Optional[Tensor] = None,
                uniform_out: Optional[Tensor] = None) -> None:
    """``eavqa_sample_pick``: one draw per row of float32 ``logits`` [B, >= V] under temperature / top-k / top-p; ``raw``, ``emitted_col``,
    ``unfinished``, ``logprob``, ``any_unfinished`` as :func:`greedy_pick`.  The uniform of row b is ``uniform_in[b]`` (float32 [B]) when
    given, else Philox4x32-10 of (``seed``, ``step``, b); ``uniform_out`` float32 [B] receives it; ``scores_out`` float32 [B, >= V]
    receives the processed scores (-inf where a token was removed)."""
    _dev(logits)
    if logits.dtype != torch.float32 or (scores_out is not None and (scores_out.dtype != torch.float32 or scores_out.shape[0] != logits.shape[0])):
        raise _lib.EavqaError("sample_pick: float32 logits (and scores_out of as many rows)")
    B = logits.shape[0]
    call("eavqa_sample_pick", B, V, _p(logits), _ld(logits), float(temperature), int(top_k), float(top_p), int(seed) & (2 ** 64 - 1),
         int(step), _p(uniform_in), _p(uniform_out), int(pad_token_id if pad_token_id is not None else 0),
         int(eos_token_id) if eos_token_id is not None else -1, _p(raw), _p(emitted_col), emitted_col.stride(0), _p(unfinished),
         _p(logprob), _p(scores_out), _ld(scores_out) if scores_out is not None else 0, _p(any_unfinished), _stream())


def logits_process(scores: Tensor, V: int, history: Optional[Tensor], cur_len: int, *, repetition_penalty: float = 1.0,
                   no_repeat_ngram_size: int = 0, eos_token_id: Optional[int] = None, suppress_eos: bool = False,
                   bad_words: Optional[Tensor] = None, bad_lens: Optional[Tensor] = None, to_logprobs: bool = False) -> None:
    """``eavqa_logits_process``: HF's repetition penalty, n-gram, bad-word and min-length rules for one step, in place on float32
    ``scores`` [R, >= V] (``to_logprobs``: on ``log_softmax(scores)``, which replaces the row first).  ``history``: int64 [R, >= cur_len]
    (any row stride), the ids so far; ``bad_words`` int32 [n_bad, width] with ``bad_lens`` int32 [n_bad], both on the device."""
    _dev(scores)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise _lib.EavqaError("logits_process: float32 scores [R, >= V] with unit column stride")
    if cur_len > 0 and (history is None or history.dtype != torch.int64 or history.dim() != 2 or history.shape[0] != scores.shape[0]
                        or history.shape[1] < cur_len or history.stride(1) != 1):
        raise _lib.EavqaError("logits_process: int64 history [R, >= cur_len] with unit column stride")
    n_bad = 0 if bad_words is None else bad_words.shape[0]
    if n_bad and (bad_lens is None or bad_words.dtype != torch.int32 or bad_lens.dtype != torch.int32 or not bad_words.is_contiguous()
                  or bad_lens.numel() != n_bad or not bad_lens.is_contiguous()):
        raise _lib.EavqaError("logits_process: contiguous int32 bad_words [n_bad, width] and bad_lens [n_bad]")
    call("eavqa_logits_process", scores.shape[0], V, _p(scores), _ld(scores), 1 if to_logprobs else 0, _p(history) if cur_len > 0 else None,
         history.stride(0) if cur_len > 0 else 0, int(cur_len), float(repetition_penalty), int(no_repeat_ngram_size),
         int(eos_token_id) if eos_token_id is not None else -1, 1 if suppress_eos else 0, _p(bad_words) if n_bad else None,
         _p(bad_lens) if n_bad else None, n_bad, bad_words.shape[1] if n_bad else 0, _stream())


def trie_constrain(scores: Tensor, V: int, history: Optional[Tensor], cur_len: int, prompt_len: int, eos_token_id: int, child_begin: Tensor,
                   child_tok: Tensor, child_node: Tensor, is_end: Tensor, *, roots: Optional[Tensor] = None, rows_per_item: int = 1,
                   to_logprobs: bool = False) -> None:
    """``eavqa_trie_constrain``: keep, in place on float32 ``scores`` [R, >= V], the columns the trie allows after the generated ids
    ``history[:, prompt_len:cur_len]`` (and eos where a member ends, or alone once a row has ended or left the set); -inf elsewhere
    (``to_logprobs``: on ``log_softmax(scores)``, which replaces the row first).  ``history``: int64 [R, >= cur_len] (any row stride).
    The trie on the device, contiguous: ``child_begin`` int32 [N + 1], ``child_tok`` / ``child_node`` int32 [E], ``is_end`` uint8 [N];
    ``roots`` int32 [R / rows_per_item] (None: node 0 for every row)."""
    _dev(scores)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise _lib.EavqaError("trie_constrain: float32 scores [R, >= V] with unit column stride")
    walked = cur_len > prompt_len
    if walked and (history is None or history.dtype != torch.int64 or history.dim() != 2 or history.shape[0] != scores.shape[0]
                   or history.shape[1] < cur_len or history.stride(1) != 1):
        raise _lib.EavqaError("trie_constrain: int64 history [R, >= cur_len] with unit column stride")
    N, E = is_end.numel(), child_tok.numel()
    if (child_begin.dtype != torch.int32 or child_tok.dtype != torch.int32 or child_node.dtype != torch.int32 or is_end.dtype != torch.uint8
            or child_begin.numel() != N + 1 or child_node.numel() != E
            or not all(t.is_contiguous() and t.device == scores.device for t in (child_begin, child_tok, child_node, is_end))):
        raise _lib.EavqaError("trie_constrain: contiguous device child_begin int32 [N + 1], child_tok / child_node int32 [E], is_end uint8 [N]")
    R = scores.shape[0]
    if rows_per_item < 1 or R % rows_per_item or (roots is not None and (roots.dtype != torch.int32 or not roots.is_contiguous()
                                                                         or roots.device != scores.device
                                                                         or roots.numel() != R // rows_per_item)):
        raise _lib.EavqaError("trie_constrain: contiguous device roots int32 [R / rows_per_item], rows_per_item >= 1 dividing R")
    call("eavqa_trie_constrain", R, V, _p(scores), _ld(scores), 1 if to_logprobs else 0, _p(history) if walked else None,
         history.stride(0) if walked else 0, int(prompt_len), int(cur_len), int(eos_token_id), _p(child_begin), _p(child_tok) if E else None,
         _p(child_node) if E else None, _p(is_end), N, E, _p(roots), int(rows_per_item), _stream())


ENSEMBLE_MODES = {"product": _lib.EAVQA_ENSEMBLE_PRODUCT, "mixture": _lib.EAVQA_ENSEMBLE_MIXTURE}
ENSEMBLE_MAX_MEMBERS = 8


def ensemble_combine(logits: Tensor, V: int, n: int, mode: str, weights: Optional[Tensor] = None, out: Optional[Tensor] = None,
                     member_lse: Optional[Tensor] = None, stats: Optional[Tensor] = None) -> Tensor:
    """``eavqa_ensemble_combine``: float32 ``logits`` [B * n, >= V], rows ordered (question, member), folded into ``out`` float32
    [B, >= V] (None: a new [B, row width of ``logits``] buffer): ``mode`` "product" - the weighted sum of the members' log_softmax - or
    "mixture" - the log of the weighted sum of their softmax.  ``weights``: float32 [n] on the device, normalised by the caller
    (:func:`~eavqa_amd.models.search.ensemble_weights`); None: 1 / n each.  ``member_lse`` float32 [B * n] receives the members'
    log-sum-exp; ``stats`` float32 [2 * B * n] is the kernel's workspace (None: allocated here).  Columns >= V are neither read nor
    written.  Returns ``out``."""
    _dev(logits)
    if mode not in ENSEMBLE_MODES:
        raise ValueError(f"ensemble mode {mode!r}: 'product' or 'mixture'")
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise _lib.EavqaError("ensemble_combine: float32 logits [B * n, >= V] with unit column stride")
    R, n = logits.shape[0], int(n)
    if n < 1 or R % n:
        raise _lib.EavqaError("ensemble_combine: n >= 1 members per question, dividing the rows of logits")
    B, dev = R // n, logits.device
    if out is None:
        out = torch.empty((B, logits.shape[1]), device=dev, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or out.device != dev:
        raise _lib.EavqaError("ensemble_combine: out float32 [B, >= V] with unit column stride, on the device of logits")
    if logits.shape[1] < V or out.shape[1] < V:
        raise _lib.EavqaError("ensemble_combine: logits and out need at least V columns")
    if weights is not None and (weights.dtype != torch.float32 or weights.numel() != n or not weights.is_contiguous() or weights.device != dev):
        raise _lib.EavqaError("ensemble_combine: contiguous device weights float32 [n]")
    if stats is None:
        stats = torch.empty(2 * R, device=dev, dtype=torch.float32)
    elif stats.dtype != torch.float32 or stats.numel() < 2 * R or not stats.is_contiguous() or stats.device != dev:
        raise _lib.EavqaError("ensemble_combine: contiguous device stats float32 [2 * B * n]")
    if member_lse is not None and (member_lse.dtype != torch.float32 or member_lse.numel() != R or not member_lse.is_contiguous()
                                   or member_lse.device != dev):
        raise _lib.EavqaError("ensemble_combine: contiguous device member_lse float32 [B * n]")
    call("eavqa_ensemble_combine", B, n, V, _p(logits), _ld(logits), ENSEMBLE_MODES[mode], _p(weights), _p(out), _ld(out), _p(stats),
         _p(member_lse), _stream())
    return out


ENSEMBLE_MAX_GROUP = 8


def ensemble_combine_groups(logits: Tensor, V: int, n: int, G: int, mode: str, weights: Optional[Tensor] = None, out: Optional[Tensor] = None,
                            member_lse: Optional[Tensor] = None, stats: Optional[Tensor] = None) -> Tensor:
    """:func:`ensemble_combine` with ``G`` rows (beams or draws) per question.  Float32 ``logits`` [B * n * G, >= V], rows ordered
    (question, member, row), folded into ``out`` float32 [B * G, >= V] (None: a new [B * G, row width of ``logits``] buffer); row
    b * G + g combines the member rows (b * n + i) * G + g.  No copy and no other kernel: for a fixed g those member rows ARE a
    (question, member) matrix of leading dimension G * ld that starts g rows into ``logits``, and the output rows b * G + g one of
    leading dimension G * ld_out that starts g rows into ``out`` - so the call is ``eavqa_ensemble_combine`` G times, on G disjoint
    sets of rows (2 * G launches, nothing between them depends on another).  ``mode`` and ``weights`` as there; 1 <= n <= 8,
    1 <= G <= 8.  ``stats`` float32 [2 * B * n * G] (workspace; None: allocated here) and ``member_lse`` float32 [B * n * G] hold one
    block of B * n member rows (question, member) per g.  Columns >= V are neither read nor written.  Returns ``out``."""
    _dev(logits)
    if mode not in ENSEMBLE_MODES:
        raise ValueError(f"ensemble mode {mode!r}: 'product' or 'mixture'")
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise _lib.EavqaError("ensemble_combine_groups: float32 logits [B * n * G, >= V] with unit column stride")
    R, n, G = logits.shape[0], int(n), int(G)
    if not 1 <= n <= ENSEMBLE_MAX_MEMBERS or not 1 <= G <= ENSEMBLE_MAX_GROUP or R % (n * G):
        raise _lib.EavqaError(f"ensemble_combine_groups: 1..{ENSEMBLE_MAX_MEMBERS} members of 1..{ENSEMBLE_MAX_GROUP} rows per question, "
                              "n * G dividing the rows of logits")
    B, dev = R // (n * G), logits.device
    if out is None:
        out = torch.empty((B * G, logits.shape[1]), device=dev, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B * G or out.stride(1) != 1 or out.device != dev:
        raise _lib.EavqaError("ensemble_combine_groups: out float32 [B * G, >= V] with unit column stride, on the device of logits")
    if logits.shape[1] < V or out.shape[1] < V or V < 1:
        raise _lib.EavqaError("ensemble_combine_groups: logits and out need at least V >= 1 columns")
    if out.data_ptr() == logits.data_ptr():
        raise _lib.EavqaError("ensemble_combine_groups: out must not be logits")
    if weights is not None and (weights.dtype != torch.float32 or weights.numel() != n or not weights.is_contiguous() or weights.device != dev):
        raise _lib.EavqaError("ensemble_combine_groups: contiguous device weights float32 [n]")
    if stats is None:
        stats = torch.empty(2 * R, device=dev, dtype=torch.float32)
    elif stats.dtype != torch.float32 or stats.numel() < 2 * R or not stats.is_contiguous() or stats.device != dev:
        raise _lib.EavqaError("ensemble_combine_groups: contiguous device stats float32 [2 * B * n * G]")
    if member_lse is not None and (member_lse.dtype != torch.float32 or member_lse.numel() != R or not member_lse.is_contiguous()
                                   or member_lse.device != dev):
        raise _lib.EavqaError("ensemble_combine_groups: contiguous device member_lse float32 [B * n * G]")
    ld, ld_out, Bn, stream = _ld(logits), _ld(out), B * n, _stream()
    p_in, p_out, p_st, p_w = logits.data_ptr(), out.data_ptr(), stats.data_ptr(), _p(weights)
    p_lse = None if member_lse is None else member_lse.data_ptr()
    for g in range(G):
        call("eavqa_ensemble_combine", B, n, V, p_in + 4 * g * ld, G * ld, ENSEMBLE_MODES[mode], p_w, p_out + 4 * g * ld_out, G * ld_out,
             p_st + 8 * g * Bn, None if p_lse is None else p_lse + 4 * g * Bn, stream)
    return out


def token_logprobs(logits: Tensor, V: int, labels: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """``eavqa_token_logprobs``: ``out[r, i] = log_softmax(logits[r, :V])[labels[r, i]]`` (0 for a label outside [0, V)); float32
    ``logits`` [R, >= V], int64 ``labels`` [R, n <= 64], both with unit column stride; ``out`` float32 [R, n]."""
    _dev(logits)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise _lib.EavqaError("token_logprobs: float32 logits [R, >= V] with unit column stride")
    if labels.dtype != torch.int64 or labels.dim() != 2 or labels.shape[0] != logits.shape[0] or (labels.stride(1) != 1 and labels.shape[1] != 1):
        raise _lib.EavqaError("token_logprobs: int64 labels [R, n] with unit column stride")
    R, n = labels.shape
    if out is None:
        out = torch.empty((R, n), device=logits.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (R, n) or (out.stride(1) != 1 and n != 1):
        raise _lib.EavqaError("token_logprobs: out float32 [R, n] with unit column stride")
    call("eavqa_token_logprobs", R, V, _p(logits), logits.stride(0), _p(labels), labels.stride(0), n, _p(out), out.stride(0), _stream())
    return out


def candidate_rank(tok_logp: Tensor, labels: Tensor, ignored_ids=(), length_penalty: float = 0.0):
    """``eavqa_candidate_rank`` over contiguous float32 ``tok_logp`` / int64 ``labels`` [B, C, T]: returns ``(scores float32 [B, C],
    n_tokens int32 [B, C], order int32 [B, C])``; ``tok_logp`` is zeroed in place where a position is not scored."""
    _dev(tok_logp)
    if (tok_logp.dtype != torch.float32 or labels.dtype != torch.int64 or tok_logp.dim() != 3 or tok_logp.shape != labels.shape
            or not (tok_logp.is_contiguous() and labels.is_contiguous())):
        raise _lib.EavqaError("candidate_rank: contiguous float32 tok_logp and int64 labels, both [B, C, T]")
    B, C, T = tok_logp.shape
    ign = torch.tensor([int(i) for i in ignored_ids], dtype=torch.int64, device=tok_logp.device) if len(ignored_ids) else None
    scores = torch.empty((B, C), device=tok_logp.device, dtype=torch.float32)
    n_tokens = torch.empty((B, C), device=tok_logp.device, dtype=torch.int32)
    order = torch.empty((B, C), device=tok_logp.device, dtype=torch.int32)
    call("eavqa_candidate_rank", B, C, T, _p(tok_logp), _p(labels), _p(ign), 0 if ign is None else ign.numel(), float(length_penalty),
         _p(scores), _p(n_tokens), _p(order), _stream())
    return scores, n_tokens, order


def attention_merge(o1: Tensor, lse1: Tensor, o2: Tensor, lse2: Tensor, B: int, C: int, T: int, H: int, hd: int,
                    out: Optional[Tensor] = None) -> Tensor:
    """``eavqa_attention_merge``: attention over the union of two key sets from the two segments' outputs and log-sum-exps.  ``o1`` /
    ``lse1``: ``attention_fwd(..., B, H, C * T, Sk1, ..., save_lse=True)`` (rows (b, c, t) over keys shared by the C continuations of
    b); ``o2`` / ``lse2``: ``attention_fwd(..., B * C, H, T, Sk2, ..., save_lse=True)``.  ``out`` defaults to ``o2`` (in place)."""
    _dev(o1)
    out = o2 if out is None else out
    if o1.dtype != o2.dtype or out.dtype != o1.dtype or lse1.dtype != torch.float32 or lse2.dtype != torch.float32:
        raise _lib.EavqaError("attention_merge: o1 / o2 / out of one dtype, float32 lse")
    if tuple(lse1.shape) != (B, H, C * T) or tuple(lse2.shape) != (B * C, H, T) or not (lse1.is_contiguous() and lse2.is_contiguous()):
        raise _lib.EavqaError("attention_merge: contiguous lse1 [B, H, C * T] and lse2 [B * C, H, T]")
    if min(o1.shape[0], o2.shape[0], out.shape[0]) < B * C * T:
        raise _lib.EavqaError("attention_merge: o1 / o2 / out need B * C * T rows")
    call("eavqa_attention_merge", dtype_id(o1.dtype), B, C, T, H, hd, _p(o1), _ld(o1), _p(lse1), _p(o2), _ld(o2), _p(lse2), _p(out), _ld(out),
         _stream())
    return out


EARLY_STOPPING = {False: 0, True: 1, "never": 2}         # eavqa_beam_step's `early_stopping` argument


class BeamState:
    """Device buffers of one beam search over ``B`` items of ``k`` beams (the state ``eavqa_beam_step`` updates in place), initialised as
    HF's ``_beam_search`` does: running scores [0, -1e9, ...], an empty pool at -1e9, every sequence = ``start`` then ``fill``."""

    def __init__(self, B: int, k: int, max_length: int, start: int, fill: int, device):
        i32 = dict(dtype=torch.int32, device=device)
        self.B, self.k, self.max_length = B, k, max_length
        self.run_scores = torch.full((B, k), -1.0e9, dtype=torch.float32, device=device)
        self.run_scores[:, 0] = 0.0
        self.run_seq = torch.full((B * k, max_length), fill, dtype=torch.int64, device=device)
        self.run_seq[:, 0] = start
        self.pool_seq = self.run_seq.clone()
        self.pool_scores = torch.full((B, k), -1.0e9, dtype=torch.float32, device=device)
        self.pool_len = torch.ones((B, k), **i32)
        self.pool_fin = torch.zeros((B, k), **i32)
        self.improve = torch.ones(B, **i32)
        self.next_tokens = torch.full((B * k,), start, dtype=torch.int64, device=device)
        self.parents = torch.arange(B * k, **i32)
        self.cont = torch.zeros(max_length + 1, **i32)           # cont[t]: the loop goes on after the step at decoder length t
        self.ws = torch.zeros(int(_lib.load().eavqa_beam_step_workspace_bytes(B, k)), dtype=torch.uint8, device=device)


def beam_step(logits: Tensor, V: int, st: BeamState, cur_len: int, eos_token_id: int, length_penalty: float = 1.0, early_stopping=False,
              prompt_len: int = 1, logprobs: bool = False) -> None:
    """One step of HF's beam search at decoder length ``cur_len`` on the device (``eavqa_beam_step``); ``logits`` float32 [B * k, >= V].
    ``logprobs``: the rows already hold (processed) log-probabilities (``eavqa_beam_step_logprobs``)."""
    _dev(logits)
    if logits.dtype != torch.float32 or logits.shape[0] != st.B * st.k:
        raise _lib.EavqaError("beam_step: float32 logits of B * k rows")
    if early_stopping not in EARLY_STOPPING:
        raise _lib.EavqaError(f"early_stopping {early_stopping!r}")
    es = EARLY_STOPPING[early_stopping]
    lp = float(length_penalty)
    L = (st.max_length - prompt_len) if (es == 2 and lp > 0.0) else (cur_len + 1 - prompt_len)
    call("eavqa_beam_step_logprobs" if logprobs else "eavqa_beam_step", st.B, st.k, V, _p(logits), _ld(logits), int(cur_len), st.max_length, int(eos_token_id),
         float((cur_len + 1 - prompt_len) ** lp), float(L ** lp), es, _p(st.next_tokens), _p(st.parents), _p(st.run_scores), _p(st.run_seq),
         _p(st.pool_seq), _p(st.pool_scores), _p(st.pool_len), _p(st.pool_fin), _p(st.improve), _p(st.cont[cur_len:cur_len + 1]), _p(st.ws),
         st.ws.numel(), _stream())


def beam_reorder(src: Tensor, dst: Tensor, parents: Tensor, t: int) -> None:
    """``dst[p, r, j] = src[p, parents[r], j]`` for j < t: K / V cache planes [n_planes, rows, t_max, inner] gathered by beam parent."""
    _dev(src)
    n_planes, rows, t_max, inner = src.shape
    if dst.shape != src.shape or dst.dtype != src.dtype or not (src.is_contiguous() and dst.is_contiguous()):
        raise _lib.EavqaError("beam_reorder: two contiguous buffers of one shape and dtype")
    call("eavqa_beam_reorder", dtype_id(src.dtype), n_planes, rows, int(t), t_max, inner, _p(src), _p(dst), rows * t_max * inner, _p(parents),
         _stream())


def adamw(param: Tensor, grad: Tensor, m: Tensor, v: Tensor, step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999,
          eps: float = 1e-8, weight_decay: float = 0.01, grad_scale: float = 1.0, shadow: Optional[Tensor] = None) -> None:
    _dev(param)
    call("eavqa_adamw", param.numel(), _p(param), _p(grad), _p(m), _p(v), int(step), float(lr), float(beta1), float(beta2),
         float(eps), float(weight_decay), float(grad_scale), dtype_id(shadow.dtype) if shadow is not None else 0, _p(shadow), _stream())


CLIP_STATE_WORDS = C.sizeof(_lib.ClipState) // 4   # eavqa_clip_state_t as 32-bit words: norm, scale_eff, inv_bc1, inv_sqrt_bc2 (float32), applied, skipped, skip, reserved (int32)


def grad_sumsq_partials(n: int) -> int:
    """Number of per-workgroup partial sums ``eavqa_grad_sumsq`` writes for ``n`` elements (host arithmetic)."""
    return int(_lib.load().eavqa_grad_sumsq_partials(int(n)))


def grad_sumsq(grad: Tensor, partials: Tensor) -> Tensor:
    """``partials`` float64 [grad_sumsq_partials(grad.numel())] <- per-workgroup sums of squares of the flat float32 gradient."""
    _dev(grad)
    if grad.dtype != torch.float32 or partials.dtype != torch.float64 or not (grad.is_contiguous() and partials.is_contiguous()):
        raise _lib.EavqaError("grad_sumsq: a contiguous float32 gradient and contiguous float64 partials")
    call("eavqa_grad_sumsq", grad.numel(), _p(grad), _p(partials), partials.numel(), _stream())
    return partials


def clip_plan(partials: Tensor, pre_scale: float, max_norm: float, bc_table: Tensor, state: Tensor) -> None:
    """``state`` (int32 [CLIP_STATE_WORDS], the bits of ``eavqa_clip_state_t``) <- norm, effective gradient scale, bias corrections of the
    next applied step from ``bc_table`` float32 [len, 2], or the skip of a non-finite gradient."""
    _dev(partials)
    if (partials.dtype != torch.float64 or bc_table.dtype != torch.float32 or bc_table.dim() != 2 or bc_table.shape[1] != 2
            or not bc_table.is_contiguous() or state.dtype != torch.int32 or state.numel() != CLIP_STATE_WORDS or not state.is_contiguous()):
        raise _lib.EavqaError("clip_plan: float64 partials, a float32 [len, 2] table and an int32 [8] state block")
    call("eavqa_clip_plan", _p(partials), partials.numel(), float(pre_scale), float(max_norm), _p(bc_table), bc_table.shape[0], _p(state),
         _stream())


def adamw_clipped(param: Tensor, grad: Tensor, m: Tensor, v: Tensor, state: Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                  eps: float = 1e-8, weight_decay: float = 0.01, shadow: Optional[Tensor] = None) -> None:
    """``adamw`` with the step number's bias corrections and the gradient scale read from ``state`` on the device (``clip_plan``)."""
    _dev(param)
    call("eavqa_adamw_clipped", param.numel(), _p(param), _p(grad), _p(m), _p(v), float(lr), float(beta1), float(beta2), float(eps),
         float(weight_decay), _p(state), dtype_id(shadow.dtype) if shadow is not None else 0, _p(shadow), _stream())


def patchify(pixels: Tensor, ps: int, dtype: torch.dtype, ldp: int) -> Tensor:
    _dev(pixels)
    B, C3, img, _ = pixels.shape
    g = img // ps
    pixels = pixels.contiguous().float()
    out = torch.empty((B * g * g, ldp), device=pixels.device, dtype=dtype)
    call("eavqa_patchify", dtype_id(dtype), B, img, ps, _p(pixels), _p(out), ldp, _stream())
    return out


def clip_resize_rows(src: Tensor, plan) -> Tensor:
    """Horizontal pass of the CLIP image preprocessing (eavqa_clip_resize_rows): ``src`` the packed uint8 bytes of the batch on the device,
    ``plan`` its ``models.clip_preprocess.PreprocessPlan``.  Returns the uint8 intermediate the vertical pass reads."""
    _dev(src)
    if src.dtype != torch.uint8 or src.numel() < plan.src_bytes:
        raise _lib.EavqaError("clip_resize_rows: src is the batch's packed uint8 buffer")
    tables, desc, tiles = plan.device_tables(src.device)
    mid = torch.empty(plan.mid_bytes, device=src.device, dtype=torch.uint8)
    call("eavqa_clip_resize_rows", plan.n_px, plan.B, tiles.shape[0], _p(src), src.numel(), _p(desc), _p(tables), tables.numel(), _p(tiles),
         _p(mid), mid.numel(), plan.mid_stride, _stream())
    return mid


def _clip_resize_emit(mid: Tensor, plan, lut: Tensor, ps: int, out: Tensor, ldp: int) -> Tensor:
    _dev(mid)
    if lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256) or not lut.is_contiguous() or lut.device != mid.device:
        raise _lib.EavqaError("clip_preprocess: lut is a contiguous float32 [3, 256] table on the images' device")
    tables, desc, _ = plan.device_tables(mid.device)
    call("eavqa_clip_resize_emit", dtype_id(out.dtype), plan.n_px, ps, plan.B, _p(desc), _p(tables), tables.numel(), _p(mid), mid.numel(),
         plan.mid_stride, _p(lut), _p(out), ldp, _stream())
    return out


def clip_preprocess(mid: Tensor, plan, lut: Tensor) -> Tensor:
    """Vertical pass + crop + normalise (eavqa_clip_resize_emit, ps = 0): float32 ``[B, 3, n_px, n_px]``."""
    out = torch.empty((plan.B, 3, plan.n_px, plan.n_px), device=mid.device, dtype=torch.float32)
    return _clip_resize_emit(mid, plan, lut, 0, out, 0)


def clip_preprocess_patches(mid: Tensor, plan, lut: Tensor, ps: int, dtype: torch.dtype, ldp: int, out: Optional[Tensor] = None) -> Tensor:
    """The same pixels written as ``patchify``'s rows: ``dtype`` ``[B * g * g, ldp]``, pad columns zero."""
    if ps <= 0:
        raise _lib.EavqaError("clip_preprocess_patches: ps must be positive")
    g = plan.n_px // ps
    if out is None:
        out = torch.empty((plan.B * g * g, ldp), device=mid.device, dtype=dtype)
    elif out.dtype != dtype or tuple(out.shape) != (plan.B * g * g, ldp) or not out.is_contiguous() or out.device != mid.device:
        raise _lib.EavqaError("clip_preprocess_patches: out is a contiguous [B * g * g, ldp] tensor of `dtype` on the images' device")
    return _clip_resize_emit(mid, plan, lut, ps, out, ldp)


def vit_assemble(patch_embed: Tensor, cls: Tensor, pos: Tensor, B: int, n_patch: int) -> Tensor:
    W = patch_embed.shape[1]
    x = torch.empty((B * (n_patch + 1), W), device=patch_embed.device, dtype=torch.float32)
    call("eavqa_vit_assemble", dtype_id(patch_embed.dtype), B, n_patch, W, _p(patch_embed), _ld(patch_embed), _p(cls), _p(pos),
         _p(x), _ld(x), _stream())
    return x


def cast_rows(x: Tensor, dtype: torch.dtype, out: Optional[Tensor] = None) -> Tensor:
    rows, cols = x.shape
    y = out if out is not None else torch.empty((rows, cols), device=x.device, dtype=dtype)
    call("eavqa_cast_rows", dtype_id(dtype), rows, cols, _p(x), _ld(x), _p(y), _ld(y), _stream())
    return y


def copy_rows(src: Tensor, dst: Tensor, B: int, S: int, cols: int, src_batch_rows: int, dst_batch_rows: int, dst_row0: int) -> None:
    """Strided row copy (KV-cache fill / append); ``src``/``dst`` are 2-D row views."""
    call("eavqa_copy_rows", dtype_id(src.dtype), B, S, cols, _p(src), _ld(src), src_batch_rows, _p(dst), _ld(dst),
         dst_batch_rows, dst_row0, _stream())


def colsum(x: Tensor, out: Tensor, accumulate: bool) -> None:
    rows, cols = x.shape
    call("eavqa_colsum", dtype_id(x.dtype), rows, cols, _p(x), _ld(x), _p(out), int(accumulate), _stream())


def transpose(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    rows, cols = x.shape
    y = out if out is not None else torch.empty((cols, rows), device=x.device, dtype=x.dtype)
    call("eavqa_transpose", dtype_id(x.dtype), rows, cols, _p(x), _ld(x), _p(y), _ld(y), _stream())
    return y


def _splitk_partials(entry: str, a: Tensor, b: Tensor, ks: Optional[int], out: Optional[Tensor]):
    """(M, N, K, ks, partial-sum buffer [ks, M, N]) of a split-K call; ``ks`` None = what ``<entry>_plan`` recommends, or raise."""
    M, K = a.shape
    N = b.shape[0]
    if ks is None:
        ks = int(getattr(_lib.load(), entry + "_plan")(M, N, K))
        if ks <= 0:
            raise _lib.EavqaError(f"{entry}: unsupported shape M={M} N={N} K={K}")
    return M, N, K, ks, out if out is not None else torch.empty((ks, M, N), device=a.device, dtype=torch.float32)


def gemm_splitk(a: Tensor, b: Tensor, ks: Optional[int] = None, unroll: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """fp32 partial sums [ks, M, N] of a [M,K] @ b [N,K]^T (bf16, M <= 64): the decode-step weight-streaming GEMM.
    ``unroll`` (tests / tools only) selects the depth of the weight-load window through ``eavqa_gemm_splitk_ex``."""
    M, N, K, ks, part = _splitk_partials("eavqa_gemm_splitk", a, b, ks, out)
    if unroll:
        call("eavqa_gemm_splitk_ex", dtype_id(a.dtype), M, N, K, _p(a), _ld(a), _p(b), _ld(b), _p(part), ks, _stream(), unroll)
    else:
        call("eavqa_gemm_splitk", dtype_id(a.dtype), M, N, K, _p(a), _ld(a), _p(b), _ld(b), _p(part), ks, _stream())
    return part


def splitk_finish(part: Tensor, outs, bias: Optional[Tensor] = None, act: str = "none", residual: Optional[Tensor] = None) -> None:
    """outs: 1..3 2-D tensors (row stride = stride(0)), each receiving N / len(outs) columns of act(sum(part) + bias) (+ residual)."""
    ks, M, N = part.shape
    o = list(outs) + [None] * (3 - len(outs))
    call("eavqa_splitk_finish", dtype_id(outs[0].dtype), M, N, _p(part), ks, _p(bias),
         _lib.ACT[act], _p(residual), residual.stride(0) if residual is not None else 0, int(outs[0].dtype == torch.float32), len(outs),
         _p(o[0]), o[0].stride(0), _p(o[1]), o[1].stride(0) if o[1] is not None else 0, _p(o[2]), o[2].stride(0) if o[2] is not None else 0,
         _stream())


def layernorm_splitk(x_in: Tensor, gamma: Tensor, beta: Tensor, eps: float, out_dtype, part: Optional[Tensor] = None,
                     bias: Optional[Tensor] = None, x_out: Optional[Tensor] = None) -> Tensor:
    rows, cols = x_in.shape
    y = torch.empty((rows, cols), device=x_in.device, dtype=out_dtype)
    call("eavqa_layernorm_splitk", dtype_id(out_dtype), rows, cols, _p(x_in), _ld(x_in), _p(part), 0 if part is None else part.shape[0],
         _p(bias), _p(x_out), _ld(x_out) if x_out is not None else 0, _p(gamma), _p(beta), float(eps), _p(y), _ld(y), _stream())
    return y


def gemm_fp8_splitk(a_q: Tensor, a_scale: Tensor, b_q: Tensor, b_scale: float, ks: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """fp32 partial sums [ks, M, N] (scales applied) of e4m3 rows ``a_q`` [M, K] x e4m3 weights ``b_q`` [N, K]^T (``eavqa_gemm_fp8_splitk``)."""
    M, N, K, ks, part = _splitk_partials("eavqa_gemm_fp8_splitk", a_q, b_q, ks, out)
    call("eavqa_gemm_fp8_splitk", M, N, K, _p(a_q), _ld(a_q), _p(a_scale), _p(b_q), _ld(b_q), float(b_scale), _p(part), ks, _stream())
    return part


def layernorm_splitk_fp8(x_in: Tensor, gamma: Tensor, beta: Tensor, eps: float, part: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                         x_out: Optional[Tensor] = None):
    """``layernorm_splitk`` whose output feeds an fp8 GEMM: (e4m3 bytes uint8 [rows, cols], float32 row scales [rows])."""
    rows, cols = x_in.shape
    yq = torch.empty((rows, cols), device=x_in.device, dtype=torch.uint8)
    sc = torch.empty(rows, device=x_in.device, dtype=torch.float32)
    call("eavqa_layernorm_splitk_fp8", rows, cols, _p(x_in), _ld(x_in), _p(part), 0 if part is None else part.shape[0], _p(bias), _p(x_out),
         _ld(x_out) if x_out is not None else 0, _p(gamma), _p(beta), float(eps), _p(yq), _ld(yq), _p(sc), _stream())
    return yq, sc


def rmsnorm_splitk(x_in: Tensor, gamma: Tensor, eps: float, out_dtype, part: Optional[Tensor] = None, x_out: Optional[Tensor] = None,
                   out: Optional[Tensor] = None) -> Tensor:
    """x = x_in + sum(part) (-> ``x_out``); returns T5LayerNorm(x) in ``out_dtype`` (``eavqa_rmsnorm_splitk``)."""
    rows, cols = x_in.shape
    y = out if out is not None else torch.empty((rows, cols), device=x_in.device, dtype=out_dtype)
    call("eavqa_rmsnorm_splitk", dtype_id(out_dtype), rows, cols, _p(x_in), _ld(x_in), _p(part), 0 if part is None else part.shape[0],
         _p(x_out), _ld(x_out) if x_out is not None else 0, _p(gamma), float(eps), _p(y), _ld(y), _stream())
    return y


def splitk_finish_gated(part: Tensor, act: str, out_dtype) -> Tensor:
    """h = act(sum(part)[:, :F]) * sum(part)[:, F:] for partial sums [ks, M, 2F] (``eavqa_splitk_finish_gated``)."""
    ks, M, N2 = part.shape
    h = torch.empty((M, N2 // 2), device=part.device, dtype=out_dtype)
    call("eavqa_splitk_finish_gated", dtype_id(out_dtype), M, N2 // 2, _p(part), ks, _lib.ACT[act], _p(h), _ld(h), _stream())
    return h


def attention_decode_splitk_rel(part: Tensor, k: Tensor, v: Tensor, B: int, H: int, Sk: int, hd: int, *, kv_batch_rows: int,
                                key_mask: Optional[Tensor] = None, scale: float = 1.0, rel_bias: Optional[Tensor] = None, rel_zero: int = 0) -> Tensor:
    """One decode step of attention whose query (and, with 3 H hd columns, new K / V row) is summed from split-K partial sums
    [ks, B, H hd | 3 H hd]; optional T5 relative-position bias table [H, ld] (``eavqa_attention_decode_splitk_rel``)."""
    ks, _, cols = part.shape
    o = torch.empty((B, H * hd), device=part.device, dtype=k.dtype)
    call("eavqa_attention_decode_splitk_rel", dtype_id(k.dtype), B, H, Sk, hd, _p(part), ks, cols, _p(k), k.stride(0), _p(v), v.stride(0),
         kv_batch_rows, _p(o), _ld(o), _p(key_mask), key_mask.stride(0) if key_mask is not None else 0, float(scale),
         _p(rel_bias), rel_bias.stride(0) if rel_bias is not None else 0, int(rel_zero), _stream())
    return o


def gemm_decode_cols(M: int, N: int, K: int, a_kind: int = 0, gated: bool = False) -> int:
    """Columns of C one workgroup of ``eavqa_gemm_decode`` owns (0: unsupported shape) - the width of one statistics partial."""
    return int(_lib.load().eavqa_gemm_decode_cols(M, N, K, a_kind, int(gated)))


def gemm_decode(a: Tensor, b: Tensor, outs, *, norm: Optional[str] = None, gamma: Optional[Tensor] = None, beta: Optional[Tensor] = None,
                eps: float = 1e-5, stats_in: Optional[Tensor] = None, stats_in_cols: int = 0, gated: bool = False,
                bias: Optional[Tensor] = None, act: str = "none", residual: Optional[Tensor] = None, want_stats: bool = False, sel: int = 0):
    """The decode-step GEMM without partial sums (``eavqa_gemm_decode``): ``outs`` (1..3 2-D tensors, bf16 or fp32) receive equal
    column segments of ``epilogue(norm(a) @ b^T)``.  ``norm``: None (``a`` bf16) | "layer" | "rms" (``a`` = the fp32 stream, ``stats_in``
    [M, n, 2] from the producing call).  ``gated``: ``b`` = [wi_0; wi_1].  Returns the statistics partials [M, n, 2] of the output rows
    when ``want_stats``.  ``sel`` (tests / tools): selector of ``eavqa_gemm_decode_ex``."""
    M, K = a.shape
    N = b.shape[0] // 2 if gated else b.shape[0]
    a_kind = {None: 0, "layer": 1, "rms": 2}[norm]
    g = _lib.DecodeGemm()
    g.M, g.N, g.K = M, N, K
    g.A, g.lda, g.a_kind = _p(a), _ld(a), a_kind
    g.gamma, g.beta, g.eps = _p(gamma), _p(beta), float(eps)
    if a_kind:
        g.stats_in, g.n_stats_in, g.stats_in_cols = _p(stats_in), stats_in.shape[1], int(stats_in_cols)
    g.B, g.ldb, g.gated_rows = _p(b), _ld(b), N if gated else 0
    g.bias, g.act = _p(bias), _lib.ACT[act]
    g.residual, g.ld_residual = _p(residual), residual.stride(0) if residual is not None else 0
    g.out_f32, g.n_seg = int(outs[0].dtype == torch.float32), len(outs)
    for i, o in enumerate(outs):
        g.out[i], g.ld_out[i] = _p(o), o.stride(0)
    stats = None
    if want_stats:
        plan = _lib.LaunchPlan()                     # one partial per workgroup of a row: the plan's grid, which has seen `sel`
        if _lib.load().eavqa_gemm_decode_route(M, N, K, a_kind, int(gated), sel, C.byref(plan)) != 0:
            raise _lib.EavqaError(f"eavqa_gemm_decode: unsupported shape M={M} N={N} K={K}")
        stats = torch.empty((M, plan.grid_x, 2), device=a.device, dtype=torch.float32)
        g.stats_out = _p(stats)
    if sel:
        call("eavqa_gemm_decode_ex", C.byref(g), _stream(), sel)
    else:
        call("eavqa_gemm_decode", C.byref(g), _stream())
    return stats


def l2_normalize_rows_(x: Tensor) -> Tensor:
    """In place, fp32 [rows, cols] (faiss.normalize_L2)."""
    if x.dtype != torch.float32:
        raise _lib.EavqaError("l2_normalize_rows_: float32 only")
    call("eavqa_l2_normalize_rows", x.shape[0], x.shape[1], _p(x), _ld(x), _stream())
    return x


def topk_rows(scores: Tensor, k: int):
    """(values float32 [rows, k] descending, indices int64 [rows, k]); ties go to the smaller column."""
    if scores.dtype != torch.float32:
        raise _lib.EavqaError("topk_rows: float32 scores only")
    rows, cols = scores.shape
    val = torch.empty((rows, k), device=scores.device, dtype=torch.float32)
    idx = torch.empty((rows, k), device=scores.device, dtype=torch.int64)
    call("eavqa_topk_rows", rows, cols, _p(scores), _ld(scores), int(k), _p(val), _p(idx), _stream())
    return val, idx


def rices_joint_scores(text_sim: Tensor, text_idx: Tensor, q2img: Tensor, train_img: Tensor, query_img: Tensor, query_row: Tensor,
                       want_img_sim: bool = False):
    """``joint[i, j] = text_sim[i, j] + <query_img[query_row[i]], train_img[q2img[text_idx[i, j]]]>`` (``eavqa_rices_joint_scores``);
    an index outside its table gives ``-inf``.  Returns ``joint`` float32 [Nq, k], or ``(joint, img_sim)``."""
    _dev(text_sim)
    if text_sim.dtype != torch.float32 or text_idx.dtype != torch.int64 or text_sim.shape != text_idx.shape or text_sim.dim() != 2:
        raise _lib.EavqaError("rices_joint_scores: text_sim float32 and text_idx int64, both [Nq, k]")
    if q2img.dtype != torch.int32 or query_row.dtype != torch.int32 or train_img.dtype != torch.float32 or query_img.dtype != torch.float32:
        raise _lib.EavqaError("rices_joint_scores: q2img / query_row int32, image matrices float32")
    Nq, k = text_sim.shape
    if query_row.numel() != Nq or train_img.dim() != 2 or query_img.dim() != 2 or train_img.shape[1] != query_img.shape[1]:
        raise _lib.EavqaError("rices_joint_scores: query_row [Nq], train_img [Ni, D], query_img [Nqi, D]")
    text_sim, text_idx, q2img, query_row = text_sim.contiguous(), text_idx.contiguous(), q2img.contiguous(), query_row.contiguous()
    joint = torch.empty((Nq, k), device=text_sim.device, dtype=torch.float32)
    img_sim = torch.empty_like(joint) if want_img_sim else None
    call("eavqa_rices_joint_scores", Nq, k, train_img.shape[1], q2img.numel(), train_img.shape[0], query_img.shape[0], _p(text_sim),
         _p(text_idx), _p(q2img), _p(train_img), _ld(train_img), _p(query_img), _ld(query_img), _p(query_row), _p(joint), _p(img_sim),
         _stream())
    return (joint, img_sim) if want_img_sim else joint


def clip_text_plan(token_ids: Tensor, pack: bool = True):
    """int64 [B, S] token ids on the GPU -> (eot int32 [B], cu_seqlens int32 [B + 1], tok_rows, pos_rows int32 [B * S] (the first
    ``cu_seqlens[-1]`` entries valid), pooled_row int32 [B]) - ``eavqa_clip_text_plan``."""
    _dev(token_ids)
    if token_ids.dtype != torch.int64 or token_ids.dim() != 2:
        raise _lib.EavqaError("clip_text_plan: int64 [B, S] token ids")
    B, S = token_ids.shape
    i32 = dict(device=token_ids.device, dtype=torch.int32)
    eot, cu, pooled = torch.empty(B, **i32), torch.empty(B + 1, **i32), torch.empty(B, **i32)
    tok, pos = torch.empty(B * S, **i32), torch.empty(B * S, **i32)
    call("eavqa_clip_text_plan", B, S, int(pack), _p(token_ids), _ld(token_ids), _p(eot), _p(cu), _p(tok), _p(pos), _p(pooled), _stream())
    return eot, cu, tok, pos, pooled


def select_rows(row_labels: Tensor, capacity: int):
    """(sel_idx int32 [capacity], sel_labels int64 [capacity], count int32 [1]) of the rows with a label >= 0, in order."""
    M = row_labels.shape[0]
    n = max(int(capacity), 1)          # capacity 0 only counts: an empty tensor has no address to hand over
    idx = torch.zeros(n, device=row_labels.device, dtype=torch.int32)
    lab = torch.full((n,), -100, device=row_labels.device, dtype=torch.int64)
    cnt = torch.zeros(1, device=row_labels.device, dtype=torch.int32)
    call("eavqa_select_rows", M, _p(row_labels), int(capacity), _p(idx), _p(lab), _p(cnt), _stream())
    return (idx, lab, cnt) if capacity else (idx[:0], lab[:0], cnt)


def gather_rows(src: Tensor, idx: Tensor) -> Tensor:
    out = torch.empty((idx.shape[0], src.shape[1]), device=src.device, dtype=src.dtype)
    call("eavqa_move_rows", dtype_id(src.dtype), 0, idx.shape[0], src.shape[1], _p(src), _ld(src), _p(idx), _p(out), _ld(out), _stream())
    return out


def scatter_rows(src: Tensor, idx: Tensor, rows: int) -> Tensor:
    """[rows, cols] zeros with out[idx[i]] = src[i]."""
    out = torch.zeros((rows, src.shape[1]), device=src.device, dtype=src.dtype)
    call("eavqa_move_rows", dtype_id(src.dtype), 1, idx.shape[0], src.shape[1], _p(src), _ld(src), _p(idx), _p(out), _ld(out), _stream())
    return out


# ----------------------------------------------------------------------------------------------------- T5 / T0 (models/t5.py)
def rmsnorm_fwd(x: Tensor, gamma: Optional[Tensor], eps: float, out_dtype: torch.dtype, save_stats: bool = False):
    """T5LayerNorm rows of ``x`` -> ``y`` in ``out_dtype`` (+ rstd)."""
    _dev(x)
    rows, cols = x.shape
    y = torch.empty((rows, cols), device=x.device, dtype=out_dtype)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32) if save_stats else None
    call("eavqa_rmsnorm_fwd", dtype_id(out_dtype), _X_KIND[x.dtype], rows, cols, _p(x), _ld(x), _p(gamma), float(eps), _p(y), _ld(y), _p(rstd), _stream())
    return (y, rstd) if save_stats else y


def rmsnorm_bwd(x: Tensor, dy: Tensor, gamma: Optional[Tensor], rstd: Tensor, dres: Optional[Tensor] = None, out: Optional[Tensor] = None,
                lowp_out: Optional[Tensor] = None) -> Tensor:
    _dev(x)
    rows, cols = x.shape
    dx = out if out is not None else torch.empty((rows, cols), device=x.device, dtype=torch.float32)
    if dres is not None and _ld(dres) != _ld(dx):
        raise _lib.EavqaError("dres must share dx's leading dimension")
    call("eavqa_rmsnorm_bwd", dtype_id(dy.dtype), _X_KIND[x.dtype], rows, cols, _p(x), _ld(x), _p(dy), _ld(dy), _p(gamma), _p(rstd), _p(dres),
         _p(dx), _ld(dx), _p(lowp_out), _ld(lowp_out) if lowp_out is not None else 0, _stream())
    return dx


def gated_act_fwd(u: Tensor, act: str) -> Tensor:
    """``u`` [rows, 2F] -> ``act(u[:, :F]) * u[:, F:]`` [rows, F]."""
    _dev(u)
    rows, F2 = u.shape
    h = torch.empty((rows, F2 // 2), device=u.device, dtype=u.dtype)
    call("eavqa_gated_act_fwd", dtype_id(u.dtype), rows, F2 // 2, ACT[act], _p(u), _ld(u), _p(h), _ld(h), _stream())
    return h


def gated_act_bwd(u: Tensor, dh: Tensor, act: str) -> Tensor:
    rows, F2 = u.shape
    du = torch.empty_like(u)
    call("eavqa_gated_act_bwd", dtype_id(u.dtype), rows, F2 // 2, ACT[act], _p(u), _ld(u), _p(dh), _ld(dh), _p(du), _ld(du), _stream())
    return du


def attention_fwd_rel(q: Tensor, k: Tensor, v: Tensor, B: int, H: int, Sq: int, Sk: int, hd: int, *, rel_bias: Optional[Tensor], rel_zero: int = 0,
                      key_mask: Optional[Tensor] = None, causal: bool = False, scale: float = 1.0, save_lse: bool = False,
                      q_batch_rows: int = 0, kv_batch_rows: int = 0, ld_mask: int = 0):
    """Attention with T5's relative-position bias table ``rel_bias`` [H, n_offsets] float32 (offset key - query at column + rel_zero)."""
    _dev(q)
    o = torch.empty((B * Sq, H * hd), device=q.device, dtype=q.dtype)
    lse = torch.empty((B, H, Sq), device=q.device, dtype=torch.float32) if save_lse else None
    if B * H > ATTN_MAX_PAIRS:
        launches = _attn_batches(B, H, Sq, Sk, q, k, v, o, key_mask, lse, q_batch_rows, kv_batch_rows, ld_mask)
    else:
        launches = ((B, _p(q), _p(k), _p(v), _p(o), _p(key_mask), _p(lse)),)
    for n, pq, pk, pv, po, pm, pl in launches:
        call("eavqa_attention_fwd_rel", dtype_id(q.dtype), n, H, Sq, Sk, hd, pq, _ld(q), pk, _ld(k), pv, _ld(v), po, _ld(o), q_batch_rows,
             kv_batch_rows, pm, ld_mask, int(causal), float(scale), _p(rel_bias), rel_bias.stride(0) if rel_bias is not None else 0,
             int(rel_zero), pl, _stream())
    return (o, lse) if save_lse else o


def attention_bwd_rel(q, k, v, o, d_o, lse, B, H, Sq, Sk, hd, *, rel_bias=None, rel_zero=0, key_mask=None, causal=False, scale=1.0,
                      dq=None, dk=None, dv=None):
    _dev(q)
    dq = dq if dq is not None else torch.empty((B * Sq, H * hd), device=q.device, dtype=q.dtype)
    dk = dk if dk is not None else torch.empty((B * Sk, H * hd), device=q.device, dtype=q.dtype)
    dv = dv if dv is not None else torch.empty((B * Sk, H * hd), device=q.device, dtype=q.dtype)
    delta = torch.empty((B, H, Sq), device=q.device, dtype=torch.float32)
    call("eavqa_attention_bwd_rel", dtype_id(q.dtype), B, H, Sq, Sk, hd, _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(o), _ld(o), _p(d_o), _ld(d_o),
         _p(dq), _ld(dq), _p(dk), _ld(dk), _p(dv), _ld(dv), _p(key_mask), int(causal), float(scale), _p(rel_bias),
         rel_bias.stride(0) if rel_bias is not None else 0, int(rel_zero), _p(lse), _p(delta), _stream())
    return dq, dk, dv


# ----------------------------------------------------------------------------------------------------- Llama family (models/lm.py; libeavqa_llama_hip.so)
def _rope_args(who: str, rows: int, pos: Tensor, cos: Tensor, sin: Tensor) -> None:
    """The C entry points take ONE ld_table for both tables and a dense pos: anything else would read other rows than the caller means."""
    if pos.numel() != rows or pos.dtype != torch.int32 or not pos.is_contiguous():
        raise _lib.EavqaError(f"{who}: pos must be contiguous int32 with one entry per row")
    if cos.dim() != 2 or cos.shape != sin.shape or _ld(cos) != _ld(sin) or cos.dtype != torch.float32 or sin.dtype != torch.float32:
        raise _lib.EavqaError(f"{who}: cos and sin must be float32 [n_pos, >= hd / 2] tables of one shape and one row stride")


def _dense_partials(who: str, part: Tensor) -> None:
    """Partial sums have no leading dimension in the C ABI: [ks][M][N] float32, dense."""
    if part.dim() != 3 or part.dtype != torch.float32 or not part.is_contiguous():
        raise _lib.EavqaError(f"{who}: the partial sums must be a contiguous float32 [ks, M, N] tensor")


def rope(x: Tensor, H: int, hd: int, pos: Tensor, cos: Tensor, sin: Tensor, inverse: bool = False) -> Tensor:
    """Rotary position embedding IN PLACE on the first ``H * hd`` columns of the rows ``x`` (``eavqa_rope``): ``pos`` int32 [rows],
    ``cos`` / ``sin`` float32 [n_pos, hd / 2]; ``inverse``: the transposed rotation (the backward, on dq / dk)."""
    _dev(x)
    rows = x.shape[0]
    _rope_args("rope", rows, pos, cos, sin)
    _lib_llama.call("eavqa_rope", dtype_id(x.dtype), rows, H, hd, _p(x), _ld(x), _p(pos), _p(cos), _p(sin), _ld(cos), cos.shape[0], int(bool(inverse)), _stream())
    return x


def swiglu_fwd(u: Tensor) -> Tensor:
    """``u`` [rows, 2F] = gate | up -> ``silu(gate) * up`` [rows, F] (``eavqa_swiglu_fwd``)."""
    _dev(u)
    rows, F2 = u.shape
    h = torch.empty((rows, F2 // 2), device=u.device, dtype=u.dtype)
    _lib_llama.call("eavqa_swiglu_fwd", dtype_id(u.dtype), rows, F2 // 2, _p(u), _ld(u), _p(h), _ld(h), _stream())
    return h


def swiglu_bwd(u: Tensor, dh: Tensor) -> Tensor:
    """d gate | d up [rows, 2F] of :func:`swiglu_fwd` (``eavqa_swiglu_bwd``)."""
    rows, F2 = u.shape
    du = torch.empty_like(u)
    _lib_llama.call("eavqa_swiglu_bwd", dtype_id(u.dtype), rows, F2 // 2, _p(u), _ld(u), _p(dh), _ld(dh), _p(du), _ld(du), _stream())
    return du


def rope_finish(part: Tensor, H: int, hd: int, pos: Tensor, cos: Tensor, sin: Tensor, out_dtype, out: Optional[Tensor] = None) -> Tensor:
    """q | k | v rows [M, 3 H hd] in ``out_dtype`` from the split-K partial sums [ks, M, 3 H hd] of a QKV product, q and k rotated by
    ``pos`` (``eavqa_rope_finish``)."""
    _dense_partials("rope_finish", part)
    ks, M, N = part.shape
    _rope_args("rope_finish", M, pos, cos, sin)
    o = out if out is not None else torch.empty((M, N), device=part.device, dtype=out_dtype)
    _lib_llama.call("eavqa_rope_finish", dtype_id(out_dtype), M, H, hd, _p(part), ks, _p(pos), _p(cos), _p(sin), _ld(cos), cos.shape[0], _p(o), _ld(o), _stream())
    return o


def swiglu_splitk(part: Tensor, out_dtype) -> Tensor:
    """h = silu(sum(part)[:, :F]) * sum(part)[:, F:] for partial sums [ks, M, 2F] (``eavqa_swiglu_splitk``)."""
    _dense_partials("swiglu_splitk", part)
    ks, M, N2 = part.shape
    h = torch.empty((M, N2 // 2), device=part.device, dtype=out_dtype)
    _lib_llama.call("eavqa_swiglu_splitk", dtype_id(out_dtype), M, N2 // 2, _p(part), ks, _p(h), _ld(h), _stream())
    return h
