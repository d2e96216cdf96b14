/*
 * eavqa_llama.h - the C ABI of libeavqa_llama_hip.so: the kernels and the layer driver that the Llama family adds to the frozen causal LM
 * (csrc/llama.hip, csrc/llama_block.cpp).  A library of its own beside libeavqa_hip.so, which it links against for every entry point of
 * include/eavqa.h its driver calls: the ABI of include/eavqa.h and the symbol table of libeavqa_hip.so stay exactly what they were.
 * Conventions (dtype codes, error codes, leading dimensions in elements, `stream` = hipStream_t, enqueue-only) are those of eavqa.h.
 * Plain C99.
 */
#ifndef EAVQA_LLAMA_H
#define EAVQA_LLAMA_H

#include "eavqa.h"

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with hidden visibility: exactly the entry points declared here are exported */
#pragma GCC visibility push(default)

/* HF:models/llama/modeling_llama.py.  RMSNorm (eavqa_rmsnorm_* of eavqa.h), rotary positions, SwiGLU, no biases.  Grouped-query attention is expanded into the QKV weight at load
 * (models/lm.py), so every kernel sees plain multi-head attention.
 * eavqa_rope: rotary position embedding IN PLACE, HF's rotate_half convention (HF:llama apply_rotary_pos_emb).  x: `dtype` [rows, ldx],
 *   H heads of hd columns from column 0; pos int32 [rows]; cos / sin float32 [n_pos, ld_table] (ld_table >= hd / 2), made on the host as
 *   HF makes them - the kernels call no sincos.  For every row r, head h, i < hd / 2 the pair (a, b) = (x[r, h hd + i],
 *   x[r, h hd + i + hd / 2]) becomes (a c - b s, b c + a s), c / s = cos / sin[pos[r], i]; inverse != 0 uses -s: the transpose of the
 *   rotation, which is its backward (applied to dq / dk).  float32 arithmetic, one rounding to `dtype`.  One call over the q | k columns of
 *   QKV rows: H = 2 * heads, ldx = 3 E.  A row whose pos lies outside [0, n_pos) is NOT rotated (left as it is); the index never becomes
 *   an address.  bfloat16 / float32 (EAVQA_E_DTYPE); hd % 8 == 0, hd <= 256, ldx >= H hd, ld_table >= hd / 2 (EAVQA_E_SHAPE); x 16-byte
 *   aligned, ldx % 8 (bfloat16) / % 4 (float32), cos / sin 16-byte aligned, ld_table % 4 (EAVQA_E_ALIGN).
 * eavqa_swiglu_fwd / _bwd: eavqa_gated_act_fwd / _bwd with silu(g) = g sigmoid(g) (LlamaMLP: down(silu(gate x) * up x)); u [rows, 2F] =
 *   gate | up of ONE GEMM against [gate_proj; up_proj].  fwd: h = silu(g) up; bwd: du[:, :F] = dh up silu'(g), du[:, F:] = dh silu(g).
 *   bfloat16 / float32 (EAVQA_E_DTYPE); F % 4 == 0, every leading dimension % 4 and no smaller than its row (EAVQA_E_SHAPE); u, h, dh and
 *   du aligned to 4 elements - 8 bytes (bfloat16) / 16 bytes (float32) - else EAVQA_E_ALIGN, returned before any launch.
 * eavqa_rope_finish: the consumer of a decode step's QKV product.  partials float32 [ks][M][3 H hd] (eavqa_gemm_splitk, columns q | k | v)
 *   are summed in slice order, q and k rotated by pos[m] (as eavqa_rope, forward; an out-of-range pos leaves the row unrotated), and
 *   q | k | v written to out [M, ld_out] in `dtype` (v: the rounded sum).  eavqa_attention_decode then takes q, k_new and v_new from that
 *   buffer, so the cache holds ROTATED keys, as HF's does.
 * eavqa_swiglu_splitk: h[m, c] = silu(sum_s P[s][m][c]) * sum_s P[s][m][F + c] (eavqa_splitk_finish_gated's shape).
 *   partials 16-byte aligned, out aligned as eavqa_swiglu_fwd's h (EAVQA_E_ALIGN, before any launch); F % 4, ld % 4, ld >= F.
 * eavqa_llama_block_forward: eavqa_lm_block_forward for this family - all `n_layer` layers (RMSNorm, QKV, rotary q / k, append to the
 *   cache [B, S_max, E], causal attention under the key mask, out-projection + residual, RMSNorm, gate | up, SwiGLU, down + residual) for
 *   Sq new positions per sample at sequence index row0.  layers: a HOST array of eavqa_llama_layer_t (weights in eavqa_gemm's b_kc
 *   layout, [out, in]).  pos int32 [B * Sq]: the position of every new
 *   row; cos / sin float32 [n_pos, hd / 2].  A bfloat16 step (Sq = 1, <= 64 rows, a split plan for the three products with K = E, hd <= 128,
 *   row0 < 3584) streams the weights split-K: eavqa_rmsnorm_splitk / eavqa_gemm_splitk / eavqa_rope_finish / eavqa_attention_decode /
 *   eavqa_swiglu_splitk (a down-projection whose K = F has no plan runs as eavqa_gemm with the residual in its epilogue); anything else
 *   takes the prefill sequence.  workspace >= eavqa_llama_block_workspace_bytes(dtype, B * Sq, E, F)
 *   (EAVQA_E_ARG below that).  Enqueue-only. */
typedef struct {
    const float* ln1_g;                         /* input_layernorm [E] */
    const void* w_qkv; const void* w_o;         /* [q; k; v] [3E, E] (K / V heads expanded to H), o_proj [E, E] */
    const float* ln2_g;                         /* post_attention_layernorm [E] */
    const void* w_gu; const void* w_down;       /* [gate_proj; up_proj] [2F, E], down_proj [E, F] */
    void* k_cache; void* v_cache;               /* [B, S_max, E] in `dtype`; K rotated */
} eavqa_llama_layer_t;
int eavqa_rope(int dtype, int rows, int H, int hd, void* x, int64_t ldx, const int32_t* pos, const float* cos, const float* sin,
               int64_t ld_table, int n_pos, int inverse, void* stream);
int eavqa_swiglu_fwd(int dtype, int rows, int F, const void* u, int64_t ldu, void* h, int64_t ldh, void* stream);
int eavqa_swiglu_bwd(int dtype, int rows, int F, const void* u, int64_t ldu, const void* dh, int64_t lddh, void* du, int64_t lddu,
                     void* stream);
int eavqa_rope_finish(int dtype, int M, int H, int hd, const float* partials, int ks, const int32_t* pos, const float* cos,
                      const float* sin, int64_t ld_table, int n_pos, void* out, int64_t ld_out, void* stream);
int eavqa_swiglu_splitk(int dtype, int M, int F, const float* partials, int ks, void* out, int64_t ld, void* stream);
int64_t eavqa_llama_block_workspace_bytes(int dtype, int rows, int E, int F);
int eavqa_llama_block_forward(int dtype, int n_layer, const eavqa_llama_layer_t* layers, int E, int H, int F, float eps, int B, int Sq,
                              int row0, int S_max, float* x, const int32_t* pos, const float* cos, const float* sin, int n_pos,
                              const int32_t* key_mask, int64_t ld_mask, void* workspace, int64_t workspace_bytes, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAVQA_LLAMA_H */
