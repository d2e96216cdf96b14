// Call recorder for the decoder block drivers (csrc/lm_block.cpp, csrc/t5_block.cpp): the twenty kernel entry points they call, defined
// with their real prototypes.  Each appends one line - its name and every argument - to trace_log and returns 0.  No HIP call, no device:
// the drivers are pure enqueue, so the recorded lines ARE what they do.  Linked into the tracer executable, these definitions take
// precedence over the library's for the drivers' calls; the two *_splitk_plan functions stay the library's own.
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "eavqa.h"

std::string trace_log;              // the calls of the current case
const char* trace_ws = nullptr;     // base of the case's workspace: pointers at or above it print as ws+<offset>

namespace {
void put(int v) { trace_log += ' ' + std::to_string(v); }
void put(int64_t v) { trace_log += ' ' + std::to_string(v); }
void put(float v) {
    char b[32];
    snprintf(b, sizeof b, " %.9g", v);
    trace_log += b;
}
void put(const void* p) {
    char b[32];
    const char* c = static_cast<const char*>(p);
    if (trace_ws && c >= trace_ws) snprintf(b, sizeof b, " ws+%zu", (size_t)(c - trace_ws));
    else snprintf(b, sizeof b, " %p", p);
    trace_log += b;
}
template <class... A> int rec(const char* name, A... a) {
    trace_log += "eavqa_";
    trace_log += name;
    (put(a), ...);
    trace_log += '\n';
    return 0;
}
}

extern "C" {
int eavqa_gemm(int dtype, int a_kc, int b_kc, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
               int out_flags, float alpha, const float* bias, int act, const void* aux_in, void* aux_out, int64_t ld_aux, const void* residual,
               int64_t ldr, void* stream) {
    return rec("gemm", dtype, a_kc, b_kc, M, N, K, A, lda, B, ldb, C, ldc, out_flags, alpha, bias, act, aux_in, aux_out, ld_aux, residual, ldr, stream);
}
int eavqa_gemm_fp8(int M, int N, int K, const void* A, int64_t lda, const float* a_row_scale, const void* B, int64_t ldb, float b_scale, void* C,
                   int64_t ldc, int out_f32, float alpha, const float* bias, int act, const void* aux_in, void* aux_out, int64_t ld_aux,
                   const float* residual, int64_t ldr, void* stream, int tile) {
    return rec("gemm_fp8", M, N, K, A, lda, a_row_scale, B, ldb, b_scale, C, ldc, out_f32, alpha, bias, act, aux_in, aux_out, ld_aux, residual, ldr,
               stream, tile);
}
int eavqa_gemm_splitk(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, float* partials, int ks,
                      void* stream) {
    return rec("gemm_splitk", dtype, M, N, K, A, lda, B, ldb, partials, ks, stream);
}
int eavqa_gemm_fp8_splitk(int M, int N, int K, const void* A, int64_t lda, const float* a_row_scale, const void* B, int64_t ldb, float b_scale,
                          float* partials, int ks, void* stream) {
    return rec("gemm_fp8_splitk", M, N, K, A, lda, a_row_scale, B, ldb, b_scale, partials, ks, stream);
}
int eavqa_layernorm_fwd(int dtype, int x_kind, int rows, int cols, const void* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                        void* y, int64_t ldy, float* mean, float* rstd, void* stream) {
    return rec("layernorm_fwd", dtype, x_kind, rows, cols, x, ldx, gamma, beta, eps, y, ldy, mean, rstd, stream);
}
int eavqa_layernorm_splitk(int dtype, int rows, int cols, const float* x_in, int64_t ldx, const float* partials, int ks, const float* bias,
                           float* x_out, int64_t ld_out, const float* gamma, const float* beta, float eps, void* y, int64_t ldy, void* stream) {
    return rec("layernorm_splitk", dtype, rows, cols, x_in, ldx, partials, ks, bias, x_out, ld_out, gamma, beta, eps, y, ldy, stream);
}
int eavqa_layernorm_splitk_fp8(int rows, int cols, const float* x_in, int64_t ldx, const float* partials, int ks, const float* bias, float* x_out,
                               int64_t ld_out, const float* gamma, const float* beta, float eps, void* yq, int64_t ldq, float* row_scale,
                               void* stream) {
    return rec("layernorm_splitk_fp8", rows, cols, x_in, ldx, partials, ks, bias, x_out, ld_out, gamma, beta, eps, yq, ldq, row_scale, stream);
}
int eavqa_rmsnorm_fwd(int dtype, int x_kind, int rows, int cols, const void* x, int64_t ldx, const float* gamma, float eps, void* y, int64_t ldy,
                      float* rstd, void* stream) {
    return rec("rmsnorm_fwd", dtype, x_kind, rows, cols, x, ldx, gamma, eps, y, ldy, rstd, stream);
}
int eavqa_rmsnorm_splitk(int dtype, int rows, int cols, const float* x_in, int64_t ldx, const float* partials, int ks, float* x_out,
                         int64_t ld_out, const float* gamma, float eps, void* y, int64_t ldy, void* stream) {
    return rec("rmsnorm_splitk", dtype, rows, cols, x_in, ldx, partials, ks, x_out, ld_out, gamma, eps, y, ldy, stream);
}
int eavqa_quantize_rows_fp8(int dtype, int rows, int cols, const void* x, int64_t ldx, void* out, int64_t ld_out, float* row_scale, void* stream) {
    return rec("quantize_rows_fp8", dtype, rows, cols, x, ldx, out, ld_out, row_scale, stream);
}
int eavqa_splitk_finish(int dtype, int M, int N, const float* partials, int ks, const float* bias, int act, const float* residual,
                        int64_t ld_residual, int out_f32, int n_seg, void* out0, int64_t ld0, void* out1, int64_t ld1, void* out2, int64_t ld2,
                        void* stream) {
    return rec("splitk_finish", dtype, M, N, partials, ks, bias, act, residual, ld_residual, out_f32, n_seg, out0, ld0, out1, ld1, out2, ld2, stream);
}
int eavqa_splitk_finish_gated(int dtype, int M, int F, const float* partials, int ks, int act, void* out, int64_t ld, void* stream) {
    return rec("splitk_finish_gated", dtype, M, F, partials, ks, act, out, ld, stream);
}
int eavqa_gated_act_fwd(int dtype, int rows, int F, int act, const void* u, int64_t ldu, void* h, int64_t ldh, void* stream) {
    return rec("gated_act_fwd", dtype, rows, F, act, u, ldu, h, ldh, stream);
}
int eavqa_copy_rows(int dtype, int B, int S, int cols, const void* src, int64_t lds, int64_t src_batch_rows, void* dst, int64_t ldd,
                    int64_t dst_batch_rows, int64_t dst_row0, void* stream) {
    return rec("copy_rows", dtype, B, S, cols, src, lds, src_batch_rows, dst, ldd, dst_batch_rows, dst_row0, stream);
}
int eavqa_attention_fwd(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                        int64_t ldv, void* o, int64_t ldo, int64_t q_batch_rows, int64_t kv_batch_rows, const int32_t* key_mask, int64_t ld_mask,
                        const int32_t* cu_seqlens, int causal, float scale, float* lse, void* stream) {
    return rec("attention_fwd", dtype, B, H, Sq, Sk, hd, q, ldq, k, ldk, v, ldv, o, ldo, q_batch_rows, kv_batch_rows, key_mask, ld_mask, cu_seqlens,
               causal, scale, lse, stream);
}
int eavqa_attention_fwd_rel(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                            int64_t ldv, void* o, int64_t ldo, int64_t q_batch_rows, int64_t kv_batch_rows, const int32_t* key_mask,
                            int64_t ld_mask, int causal, float scale, const float* rel_bias, int64_t rel_ld, int rel_zero, float* lse,
                            void* stream) {
    return rec("attention_fwd_rel", dtype, B, H, Sq, Sk, hd, q, ldq, k, ldk, v, ldv, o, ldo, q_batch_rows, kv_batch_rows, key_mask, ld_mask, causal,
               scale, rel_bias, rel_ld, rel_zero, lse, stream);
}
int eavqa_attention_decode(int dtype, int B, int H, int Sk, int hd, const void* q, int64_t ldq, void* k_cache, int64_t ldk, void* v_cache,
                           int64_t ldv, int64_t kv_batch_rows, const void* k_new, const void* v_new, int64_t ld_new, void* o, int64_t ldo,
                           const int32_t* key_mask, int64_t ld_mask, float scale, void* stream) {
    return rec("attention_decode", dtype, B, H, Sk, hd, q, ldq, k_cache, ldk, v_cache, ldv, kv_batch_rows, k_new, v_new, ld_new, o, ldo, key_mask,
               ld_mask, scale, stream);
}
int eavqa_attention_decode_splitk(int dtype, int B, int H, int Sk, int hd, const float* qkv_partials, int ks, const float* qkv_bias, void* k_cache,
                                  int64_t ldk, void* v_cache, int64_t ldv, int64_t kv_batch_rows, void* o, int64_t ldo, const int32_t* key_mask,
                                  int64_t ld_mask, float scale, void* stream) {
    return rec("attention_decode_splitk", dtype, B, H, Sk, hd, qkv_partials, ks, qkv_bias, k_cache, ldk, v_cache, ldv, kv_batch_rows, o, ldo,
               key_mask, ld_mask, scale, stream);
}
int eavqa_attention_decode_splitk_rel(int dtype, int B, int H, int Sk, int hd, const float* partials, int ks, int part_cols, void* k, int64_t ldk,
                                      void* v, int64_t ldv, int64_t kv_batch_rows, void* o, int64_t ldo, const int32_t* key_mask, int64_t ld_mask,
                                      float scale, const float* rel_bias, int64_t rel_ld, int rel_zero, void* stream) {
    return rec("attention_decode_splitk_rel", dtype, B, H, Sk, hd, partials, ks, part_cols, k, ldk, v, ldv, kv_batch_rows, o, ldo, key_mask, ld_mask,
               scale, rel_bias, rel_ld, rel_zero, stream);
}
int eavqa_attention_decode_shared(int dtype, int B, int G, int H, int S0, int t, int t_max, int hd, const void* q, int64_t ldq, const void* k_prompt,
                                  int64_t ldk, const void* v_prompt, int64_t ldv, int64_t prompt_batch_rows, void* k_tail, void* v_tail,
                                  int64_t ld_tail, const void* k_new, const void* v_new, int64_t ld_new, void* o, int64_t ldo,
                                  const int32_t* key_mask, int64_t ld_mask, float scale, void* stream) {
    return rec("attention_decode_shared", dtype, B, G, H, S0, t, t_max, hd, q, ldq, k_prompt, ldk, v_prompt, ldv, prompt_batch_rows, k_tail, v_tail,
               ld_tail, k_new, v_new, ld_new, o, ldo, key_mask, ld_mask, scale, stream);
}
}
