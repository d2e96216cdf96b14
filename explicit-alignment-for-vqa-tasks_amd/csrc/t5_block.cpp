// Host-side driver: ONE cached greedy step through all decoder layers of a frozen T5 (eavqa_t5_decoder_step in include/eavqa.h) -
// the calls of FrozenT5.decode_step (models/t5.py) in the same order on the same kernels, enqueued from C++ instead of ~340 ctypes
// calls per step (3 ms of Python for ~2.2 ms of GPU work on T0_3B).  Pure enqueue: no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "block_ws.h"
#include "eavqa.h"
#include "eavqa_test.h"

namespace {
using eavqa_block::Arena;

// Split-K route (round 4): every projection of the step streams its weights once with K cut over workgroups (eavqa_gemm_splitk) and its
// consumer adds the partial sums up - the RMSNorm pass (residual + finish + norm in one kernel), the decode attention (q, and the new K / V
// row it appends, summed from the partial sums), the gated finish.  12 kernels per layer instead of 14, the six GEMMs at 3-4 TB/s instead
// of the M <= 64 tile kernels' 1.3 (T0_3B, B = 32: 3.1 -> about 2.2 ms per step).
// The SHAPE part of its plan - bf16, B <= 64, shapes every split plan accepts - fixes the five split counts and the size of the partial-sum
// buffer, so the workspace size depends on it alone; whether a step may take the route is decided at run time (t5_splitk_eligible).
struct T5Plan { int qkv, o, qc, wi, wo; bool ok; size_t part_bytes; };
inline T5Plan plan_t5(int dtype, int B, int E, int I, int F, int gated) {
    T5Plan p{0, 0, 0, 0, 0, false, 0};
    if (dtype != EAVQA_BF16 || B > 64 || E % 8 || I % 8 || F % 4) return p;
    const int NI = (gated ? 2 : 1) * F;
    p.qkv = eavqa_gemm_splitk_plan(B, 3 * I, E);
    p.o = eavqa_gemm_splitk_plan(B, E, I);
    p.qc = eavqa_gemm_splitk_plan(B, I, E);
    p.wi = eavqa_gemm_splitk_plan(B, NI, E);
    p.wo = eavqa_gemm_splitk_plan(B, E, F);
    p.ok = p.qkv > 0 && p.o > 0 && p.qc > 0 && p.wi > 0 && p.wo > 0;
    size_t m = (size_t)p.qkv * 3 * I;
    const size_t c[] = {(size_t)p.o * E, (size_t)p.qc * I, (size_t)p.wi * NI, (size_t)p.wo * E};
    for (size_t v : c) m = v > m ? v : m;
    p.part_bytes = m * B * 4;
    return p;
}
inline bool t5_splitk_eligible(int I, int H, int t, int S, const float* rel_bias) {
    return H > 0 && (I / H) % 8 == 0 && I / H <= 128 && t <= 3584 && S <= 3584 && rel_bias;
}

// The workspace of a cached step on R decoder rows (greedy: R = B; beams: R = B * beams), part_bytes of split-K partial sums at its end
// (0: none; one buffer, producer and consumer alternate).
struct T5Ws { void* a; char* qkv; void* ctx; void* qc; float* x1; float* x2; void* u; void* h; float* part; };
inline T5Ws t5_layout(Arena& A, int dtype, size_t R, int E, int I, int F, int gated, size_t part_bytes) {
    const size_t es = dtype == EAVQA_BF16 ? 2 : 4;
    T5Ws w{};
    w.a = A.take(R * E * es);                           // RMSNorm output (operand of the next GEMM)
    w.qkv = A.take<char>(R * 3 * I * es);               // q | k | v of the new position
    w.ctx = A.take(R * I * es);                         // attention output (self, then cross)
    w.qc = A.take(R * I * es);                          // cross-attention query
    w.x1 = A.take<float>(R * E * 4);                    // residual stream after self / cross attention (float32)
    w.x2 = A.take<float>(R * E * 4);
    w.u = A.take(R * (gated ? 2 : 1) * F * es);         // FFN up-projection ([wi_0 x | wi_1 x] when gated)
    w.h = A.take(R * F * es);                           // gated activation
    if (part_bytes) w.part = A.take<float>(part_bytes);
    return w;
}
}

extern "C" int64_t eavqa_t5_decoder_step_workspace_bytes(int dtype, int B, int E, int inner, int F, int gated) {
    const T5Plan p = plan_t5(dtype, B, E, inner, F, gated);
    Arena count(nullptr);
    t5_layout(count, dtype, B, E, inner, F, gated, p.ok ? p.part_bytes : 0);
    return (int64_t)count.used;
}

// The eavqa_gemm route of a cached step on R = B * beams decoder rows (beams = 1: greedy).  Rows are ordered (b, beam).
static int t5_plain_route(int dtype, int n_layer, const eavqa_t5_dec_layer_t* layers, const float* ln_final, int E, int I, int H, int F, int gated,
                          int act, float eps, int B, int beams, int t, int t_max, int S, float* x, void* out, const int32_t* enc_mask,
                          int64_t ld_mask, const float* rel_bias, int64_t rel_ld, int rel_zero, const T5Ws& w, void* stream) {
    const size_t es = dtype == EAVQA_BF16 ? 2 : 4;
    const int dkv = I / H, R = B * beams, xk = 1;              // x_kind of eavqa_rmsnorm_fwd: the residual stream is float32
    int rc;
    for (int l = 0; l < n_layer; ++l) {
        const eavqa_t5_dec_layer_t& L = layers[l];
        // self-attention: the new position's q / k / v, K and V appended to the cache at row t - 1, one query at the end of t keys
        if ((rc = eavqa_rmsnorm_fwd(dtype, xk, R, E, x, E, L.ln_sa, eps, w.a, E, nullptr, stream))) return rc;
        if ((rc = eavqa_gemm(dtype, 1, 1, R, 3 * I, E, w.a, E, L.w_qkv, E, w.qkv, 3 * I, 0, 1.f, nullptr, EAVQA_ACT_NONE, nullptr, nullptr, 0, nullptr, 0, stream))) return rc;
        if ((rc = eavqa_copy_rows(dtype, R, 1, I, w.qkv + (size_t)I * es, 3 * I, 1, L.k_cache, I, t_max, t - 1, stream))) return rc;
        if ((rc = eavqa_copy_rows(dtype, R, 1, I, w.qkv + (size_t)2 * I * es, 3 * I, 1, L.v_cache, I, t_max, t - 1, stream))) return rc;
        if ((rc = eavqa_attention_fwd_rel(dtype, R, H, 1, t, dkv, w.qkv, 3 * I, L.k_cache, I, L.v_cache, I, w.ctx, I, 1, t_max, nullptr, 0, 1, 1.f,
                                          rel_bias, rel_ld, rel_zero, nullptr, stream))) return rc;
        if ((rc = eavqa_gemm(dtype, 1, 1, R, E, I, w.ctx, I, L.w_o, I, w.x1, E, EAVQA_GEMM_OUT_F32, 1.f, nullptr, EAVQA_ACT_NONE, nullptr, nullptr, 0, x, E, stream))) return rc;
        // cross-attention over the encoder output (K / V of every layer computed once by the caller): the `beams` rows of an item are the
        // query rows of ONE batch entry, so B * beams decoder rows read the B encoder outputs
        if ((rc = eavqa_rmsnorm_fwd(dtype, xk, R, E, w.x1, E, L.ln_ca, eps, w.a, E, nullptr, stream))) return rc;
        if ((rc = eavqa_gemm(dtype, 1, 1, R, I, E, w.a, E, L.w_q_ca, E, w.qc, I, 0, 1.f, nullptr, EAVQA_ACT_NONE, nullptr, nullptr, 0, nullptr, 0, stream))) return rc;
        const char* ckv = static_cast<const char*>(L.cross_kv);
        if ((rc = eavqa_attention_fwd_rel(dtype, B, H, beams, S, dkv, w.qc, I, ckv, 2 * I, ckv + (size_t)I * es, 2 * I, w.ctx, I, 0, 0, enc_mask, ld_mask, 0, 1.f,
                                          nullptr, 0, 0, nullptr, stream))) return rc;
        if ((rc = eavqa_gemm(dtype, 1, 1, R, E, I, w.ctx, I, L.w_o_ca, I, w.x2, E, EAVQA_GEMM_OUT_F32, 1.f, nullptr, EAVQA_ACT_NONE, nullptr, nullptr, 0, w.x1, E, stream))) return rc;
        // feed-forward
        if ((rc = eavqa_rmsnorm_fwd(dtype, xk, R, E, w.x2, E, L.ln_ff, eps, w.a, E, nullptr, stream))) return rc;
        if (gated) {
            if ((rc = eavqa_gemm(dtype, 1, 1, R, 2 * F, E, w.a, E, L.w_i, E, w.u, 2 * F, 0, 1.f, nullptr, EAVQA_ACT_NONE, nullptr, nullptr, 0, nullptr, 0, stream))) return rc;
            if ((rc = eavqa_gated_act_fwd(dtype, R, F, act, w.u, 2 * F, w.h, F, stream))) return rc;
        } else {
            if ((rc = eavqa_gemm(dtype, 1, 1, R, F, E, w.a, E, L.w_i, E, w.h, F, 0, 1.f, nullptr, act, nullptr, nullptr, 0, nullptr, 0, stream))) return rc;
        }
        if ((rc = eavqa_gemm(dtype, 1, 1, R, E, F, w.h, F, L.w_o_ff, F, x, E, EAVQA_GEMM_OUT_F32, 1.f, nullptr, EAVQA_ACT_NONE, nullptr, nullptr, 0, w.x2, E, stream))) return rc;
    }
    return eavqa_rmsnorm_fwd(dtype, xk, R, E, x, E, ln_final, eps, out, E, nullptr, stream);
}

static int t5_decoder_step_impl(int dtype, int n_layer, const eavqa_t5_dec_layer_t* layers, const float* ln_final, int E, int inner, int H,
                                int F, int gated, int act, float eps, int B, int t, int t_max, int S, float* x, void* out,
                                const int32_t* enc_mask, int64_t ld_mask, const float* rel_bias, int64_t rel_ld, int rel_zero,
                                void* workspace, int64_t workspace_bytes, void* stream, int route) {
    if (!layers || !ln_final || !x || !out || !workspace || n_layer <= 0 || B <= 0 || t <= 0 || t > t_max || S <= 0) return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (inner % H) return EAVQA_E_SHAPE;
    const size_t es = dtype == EAVQA_BF16 ? 2 : 4;
    const int dkv = inner / H, I = inner;
    const T5Plan P = plan_t5(dtype, B, E, I, F, gated);
    Arena arena(workspace);
    const T5Ws w = t5_layout(arena, dtype, B, E, I, F, gated, P.ok ? P.part_bytes : 0);
    if (workspace_bytes < (int64_t)arena.used) return EAVQA_E_ARG;
    int rc;
    if (P.ok && route != 1 && t5_splitk_eligible(I, H, t, S, rel_bias)) {
        const int NI = (gated ? 2 : 1) * F;
        for (int l = 0; l < n_layer; ++l) {
            const eavqa_t5_dec_layer_t& L = layers[l];
            // x = x2 + sum(feed-forward partials of the previous layer); a = RMSNorm(x)
            if (l == 0) rc = eavqa_rmsnorm_splitk(dtype, B, E, x, E, nullptr, 0, nullptr, 0, L.ln_sa, eps, w.a, E, stream);
            else rc = eavqa_rmsnorm_splitk(dtype, B, E, w.x2, E, w.part, P.wo, x, E, L.ln_sa, eps, w.a, E, stream);
            if (rc) return rc;
            // self-attention: q and the new K / V row summed from the QKV partial sums, K / V appended at row t - 1, bias of offsets -(t-1) .. 0
            if ((rc = eavqa_gemm_splitk(dtype, B, 3 * I, E, w.a, E, L.w_qkv, E, w.part, P.qkv, stream))) return rc;
            if ((rc = eavqa_attention_decode_splitk_rel(dtype, B, H, t, dkv, w.part, P.qkv, 3 * I, L.k_cache, I, L.v_cache, I, t_max, w.ctx, I, nullptr, 0, 1.f,
                                                        rel_bias, rel_ld, rel_zero, stream))) return rc;
            if ((rc = eavqa_gemm_splitk(dtype, B, E, I, w.ctx, I, L.w_o, I, w.part, P.o, stream))) return rc;
            if ((rc = eavqa_rmsnorm_splitk(dtype, B, E, x, E, w.part, P.o, w.x1, E, L.ln_ca, eps, w.a, E, stream))) return rc;
            // cross-attention: q summed from its partial sums, K / V of the encoder output
            if ((rc = eavqa_gemm_splitk(dtype, B, I, E, w.a, E, L.w_q_ca, E, w.part, P.qc, stream))) return rc;
            char* ckv = static_cast<char*>(const_cast<void*>(L.cross_kv));
            if ((rc = eavqa_attention_decode_splitk_rel(dtype, B, H, S, dkv, w.part, P.qc, I, ckv, 2 * I, ckv + (size_t)I * es, 2 * I, S, w.ctx, I, enc_mask, ld_mask,
                                                        1.f, nullptr, 0, 0, stream))) return rc;
            if ((rc = eavqa_gemm_splitk(dtype, B, E, I, w.ctx, I, L.w_o_ca, I, w.part, P.o, stream))) return rc;
            if ((rc = eavqa_rmsnorm_splitk(dtype, B, E, w.x1, E, w.part, P.o, w.x2, E, L.ln_ff, eps, w.a, E, stream))) return rc;
            // feed-forward
            if ((rc = eavqa_gemm_splitk(dtype, B, NI, E, w.a, E, L.w_i, E, w.part, P.wi, stream))) return rc;
            if (gated) rc = eavqa_splitk_finish_gated(dtype, B, F, w.part, P.wi, act, w.h, F, stream);
            else rc = eavqa_splitk_finish(dtype, B, F, w.part, P.wi, nullptr, act, nullptr, 0, 0, 1, w.h, F, nullptr, 0, nullptr, 0, stream);
            if (rc) return rc;
            if ((rc = eavqa_gemm_splitk(dtype, B, E, F, w.h, F, L.w_o_ff, F, w.part, P.wo, stream))) return rc;
        }
        // out = RMSNorm(x2 + sum(last feed-forward partials))
        return eavqa_rmsnorm_splitk(dtype, B, E, w.x2, E, w.part, P.wo, nullptr, 0, ln_final, eps, out, E, stream);
    }
    return t5_plain_route(dtype, n_layer, layers, ln_final, E, I, H, F, gated, act, eps, B, 1, t, t_max, S, x, out, enc_mask, ld_mask, rel_bias, rel_ld,
                          rel_zero, w, stream);
}

extern "C" int eavqa_t5_decoder_step(int dtype, int n_layer, const eavqa_t5_dec_layer_t* layers, const float* ln_final, int E, int inner, int H,
                                     int F, int gated, int act, float eps, int B, int t, int t_max, int S, float* x, void* out,
                                     const int32_t* enc_mask, int64_t ld_mask, const float* rel_bias, int64_t rel_ld, int rel_zero,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    return t5_decoder_step_impl(dtype, n_layer, layers, ln_final, E, inner, H, F, gated, act, eps, B, t, t_max, S, x, out, enc_mask, ld_mask, rel_bias,
                                rel_ld, rel_zero, workspace, workspace_bytes, stream, 0);
}

extern "C" int eavqa_t5_decoder_step_ex(int dtype, int n_layer, const eavqa_t5_dec_layer_t* layers, const float* ln_final, int E, int inner, int H,
                                        int F, int gated, int act, float eps, int B, int t, int t_max, int S, float* x, void* out,
                                        const int32_t* enc_mask, int64_t ld_mask, const float* rel_bias, int64_t rel_ld, int rel_zero,
                                        void* workspace, int64_t workspace_bytes, void* stream, int route) {
    return t5_decoder_step_impl(dtype, n_layer, layers, ln_final, E, inner, H, F, gated, act, eps, B, t, t_max, S, x, out, enc_mask, ld_mask, rel_bias,
                                rel_ld, rel_zero, workspace, workspace_bytes, stream, route);
}

// ---- beam search: B * beams decoder rows over B encoder outputs (the eavqa_gemm route; the split-K route needs a query-row -> K / V-batch
// mapping in eavqa_attention_decode_splitk_rel first)
extern "C" int64_t eavqa_t5_decoder_step_beams_workspace_bytes(int dtype, int B, int beams, int E, int inner, int F, int gated) {
    if (B <= 0 || beams <= 0 || E <= 0 || inner <= 0 || F <= 0) return 0;
    Arena count(nullptr);
    t5_layout(count, dtype, (size_t)B * beams, E, inner, F, gated, 0);
    return (int64_t)count.used;
}

extern "C" int eavqa_t5_decoder_step_beams(int dtype, int n_layer, const eavqa_t5_dec_layer_t* layers, const float* ln_final, int E, int inner,
                                           int H, int F, int gated, int act, float eps, int B, int beams, int t, int t_max, int S, float* x,
                                           void* out, const int32_t* enc_mask, int64_t ld_mask, const float* rel_bias, int64_t rel_ld,
                                           int rel_zero, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!layers || !ln_final || !x || !out || !workspace || n_layer <= 0 || B <= 0 || t <= 0 || t > t_max || S <= 0) return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (beams < 1 || beams > 8 || H <= 0 || inner % H || E <= 0 || F <= 0) return EAVQA_E_SHAPE;
    Arena arena(workspace);
    const T5Ws w = t5_layout(arena, dtype, (size_t)B * beams, E, inner, F, gated, 0);
    if (workspace_bytes < (int64_t)arena.used) return EAVQA_E_ARG;
    return t5_plain_route(dtype, n_layer, layers, ln_final, E, inner, H, F, gated, act, eps, B, beams, t, t_max, S, x, out, enc_mask, ld_mask,
                          rel_bias, rel_ld, rel_zero, w, stream);
}
