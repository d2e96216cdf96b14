// Host-side drivers: all decoder layers of a frozen causal LM in ONE C call (eavqa_lm_block_forward, _step_shared and _forward_fp8 in
// include/eavqa.h).  Used by generation (prefill: Sq = prompt length, decode: Sq = 1): a decode step is 9 short kernels per layer, and
// enqueueing them from Python one by one made the step host-bound (5 ms of Python for ~2 ms of GPU work on OPT-2.7B).  Pure enqueue: no
// allocation (the caller passes a workspace), no synchronisation, graph-capturable.
// Structure: one workspace layout (lm_layout), one split plan (plan_split), and two layer loops - plain_loop (norm, QKV, attention,
// out-projection + residual, norm, FFN up, FFN down + residual) and splitk_loop (the same with fp32 partial sums between producer and
// consumer).  The entry points differ in HOW a projection and the attention are issued: small policy structs, inlined into the loops.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "block_ws.h"
#include "eavqa.h"

namespace {
using eavqa_block::Arena;
enum Proj { QKV, O, FC1, FC2 };

// Split counts of a decode step's four projections (one new position per sample, at most 64 rows, every shape plannable) and its two
// partial-sum regions in floats: `scratch` serves QKV, out-projection and FFN-up in turn, `down` holds the FFN-down partial sums until the
// next layer's LayerNorm.  plan / div: eavqa_gemm_splitk_plan and 4 (bf16), eavqa_gemm_fp8_splitk_plan and 16 (e4m3).
struct SplitPlan { int qkv, o, fc1, fc2; bool ok; size_t scratch, down; };
inline SplitPlan plan_split(int (*plan)(int, int, int), int div, int rows, int E, int F) {
    SplitPlan d{};
    if (rows > 64 || E % div || F % div) return d;
    d.qkv = plan(rows, 3 * E, E), d.o = plan(rows, E, E), d.fc1 = plan(rows, F, E), d.fc2 = plan(rows, E, F);
    d.ok = d.qkv > 0 && d.o > 0 && d.fc1 > 0 && d.fc2 > 0;
    const size_t a = (size_t)d.qkv * 3 * E, b = (size_t)d.o * E, c = (size_t)d.fc1 * F;
    d.scratch = (a > b ? (a > c ? a : c) : (b > c ? b : c)) * rows;
    d.down = (size_t)d.fc2 * rows * E;
    return d;
}

// The workspace of all three drivers.  Forward: the activations, then (bf16, <= 64 rows: may be a decode step) the partial sums.  Shared:
// the activations, then the partial sums of the one product it splits.  Fp8: the Forward layout for bf16 - its partial-sum region is
// reserved and NOT used by the fp8 route - followed by the e4m3 operand, its row scales and the fp8 partial sums.
enum class Family { Forward, Shared, Fp8 };
struct LmWs {
    void* a; char* qkv; void* ctx; float* x1; void* f;    // LayerNorm output, q | k | v, attention output, fp32 residual after attention, FFN activation
    SplitPlan plan; float* part; float* down;             // the route's split counts (Shared: qkv alone) and partial sums
    void* aq; float* asc;                                 // Fp8: a quantised operand (e4m3 bytes) and its row scales
};
inline LmWs lm_layout(Arena& A, Family fam, int dtype, int rows, int E, int F) {
    const size_t es = dtype == EAVQA_BF16 ? 2 : 4, R = rows;
    LmWs w{};
    w.a = A.take(R * E * es);
    w.qkv = A.take<char>(R * 3 * E * es);
    w.ctx = A.take(R * E * es);
    w.x1 = A.take<float>(R * E * 4);
    w.f = A.take(R * F * es);
    auto partials = [&](const SplitPlan& p) {
        w.plan = p;
        w.part = p.ok ? A.take<float>(p.scratch * 4) : nullptr;
        w.down = p.ok ? A.take<float>(p.down * 4) : nullptr;
    };
    if (fam == Family::Shared) {
        if (dtype == EAVQA_BF16 && rows <= 64 && E % 4 == 0) w.plan.qkv = eavqa_gemm_splitk_plan(rows, 3 * E, E);
        if (w.plan.qkv > 0) w.part = A.take<float>((size_t)w.plan.qkv * R * 3 * E * 4);
        return w;
    }
    if (dtype == EAVQA_BF16) partials(plan_split(eavqa_gemm_splitk_plan, 4, rows, E, F));
    if (fam == Family::Fp8) {
        w.aq = A.take(R * (F > 3 * E ? F : 3 * E));
        w.asc = A.take<float>(R * 4);
        partials(plan_split(eavqa_gemm_fp8_splitk_plan, 16, rows, E, F));
    }
    return w;
}
inline int64_t lm_bytes(Family fam, int dtype, int rows, int E, int F) {
    Arena count(nullptr);
    lm_layout(count, fam, dtype, rows, E, F);
    return (int64_t)count.used;
}

struct Block {      // what every call of a layer loop needs
    int dtype, n_layer; const eavqa_lm_layer_t* layers; int E, H, F, act; float eps; int B, rows; float* x; const int32_t* key_mask;
    int64_t ld_mask; void* stream;
    int hd() const { return E / H; }
    float scale() const { return 1.0f / sqrtf((float)hd()); }
    size_t es() const { return dtype == EAVQA_BF16 ? 2 : 4; }
};
inline float scale_of(const eavqa_lm_layer_scales_t& s, Proj p) { return p == QKV ? s.s_qkv : p == O ? s.s_o : p == FC1 ? s.s_fc1 : s.s_fc2; }
inline bool attends_from_partials(int hd, int Sk, int E) { return hd % 8 == 0 && hd <= 128 && Sk <= 3584 && E % 8 == 0; }

// ---- plain_loop policies.  A projection: C [rows, N] = act(A [rows, K] x W^T + bias) (+ res); with a residual C is the fp32 stream.
struct Gemm {               // eavqa_gemm; ks_qkv > 0 (shared step): the QKV product through the split-K kernel + finish pass instead
    int ks_qkv;
    int operator()(const Block& b, const LmWs& w, int, Proj p, int N, int K, const void* A, const void* W, const float* bias, int act, void* C,
                   const float* res) const {
        if (p == QKV && ks_qkv > 0) {
            if (int rc = eavqa_gemm_splitk(b.dtype, b.rows, N, K, A, K, W, K, w.part, ks_qkv, b.stream)) return rc;
            return eavqa_splitk_finish(b.dtype, b.rows, N, w.part, ks_qkv, bias, act, nullptr, 0, 0, 1, C, N, nullptr, 0, nullptr, 0, b.stream);
        }
        return eavqa_gemm(b.dtype, 1, 1, b.rows, N, K, A, K, W, K, C, N, res || b.dtype == EAVQA_F32, 1.f, bias, act, nullptr, nullptr, 0, res,
                          res ? N : 0, b.stream);
    }
};
struct GemmFp8 {            // the calls of FrozenCausalLM.forward's `linear()`: quantise the rows, multiply on the fp8 cores
    const eavqa_lm_layer_scales_t* scales;
    int operator()(const Block& b, const LmWs& w, int l, Proj p, int N, int K, const void* A, const void* W, const float* bias, int act, void* C,
                   const float* res) const {
        if (int rc = eavqa_quantize_rows_fp8(b.dtype, b.rows, K, A, K, w.aq, K, w.asc, b.stream)) return rc;
        return eavqa_gemm_fp8(b.rows, N, K, w.aq, K, w.asc, W, K, scale_of(scales[l], p), C, N, res != nullptr, 1.f, bias, act, nullptr, nullptr, 0,
                              res, res ? N : 0, b.stream, 0);
    }
};
struct AppendAttn {         // append K / V of the Sq new positions to the cache [B, S_max, E], then attend positions [0, row0 + Sq)
    int Sq, row0, S_max;
    int operator()(const Block& b, const LmWs& w, int l) const {
        const eavqa_lm_layer_t& L = b.layers[l];
        const int E = b.E;
        if (int rc = eavqa_copy_rows(b.dtype, b.B, Sq, E, w.qkv + (size_t)E * b.es(), 3 * E, Sq, L.k_cache, E, S_max, row0, b.stream)) return rc;
        if (int rc = eavqa_copy_rows(b.dtype, b.B, Sq, E, w.qkv + (size_t)2 * E * b.es(), 3 * E, Sq, L.v_cache, E, S_max, row0, b.stream)) return rc;
        return eavqa_attention_fwd(b.dtype, b.B, b.H, Sq, row0 + Sq, b.hd(), w.qkv, 3 * E, L.k_cache, E, L.v_cache, E, w.ctx, E, Sq, S_max, b.key_mask,
                                   b.ld_mask, nullptr, 1, b.scale(), nullptr, b.stream);
    }
};
struct SharedAttn {         // G rows per prompt: the prompt caches stay B planes, the kernel appends to the per-row tails
    const eavqa_lm_tail_t* tails; int G, S0, S_max, t, t_max;
    int operator()(const Block& b, const LmWs& w, int l) const {
        const eavqa_lm_layer_t& L = b.layers[l];
        const int E = b.E;
        return eavqa_attention_decode_shared(b.dtype, b.B, G, b.H, S0, t, t_max, b.hd(), w.qkv, 3 * E, L.k_cache, E, L.v_cache, E, S_max, tails[l].k_tail,
                                             tails[l].v_tail, E, w.qkv + (size_t)E * b.es(), w.qkv + (size_t)2 * E * b.es(), 3 * E, w.ctx, E, b.key_mask,
                                             b.ld_mask, b.scale(), b.stream);
    }
};

template <class P, class A> int plain_loop(const Block& b, const LmWs& w, const P& proj, const A& attn) {
    const int E = b.E, F = b.F;
    int rc;
    for (int l = 0; l < b.n_layer; ++l) {
        const eavqa_lm_layer_t& L = b.layers[l];
        if ((rc = eavqa_layernorm_fwd(b.dtype, 1, b.rows, E, b.x, E, L.ln1_g, L.ln1_b, b.eps, w.a, E, nullptr, nullptr, b.stream))) return rc;
        if ((rc = proj(b, w, l, QKV, 3 * E, E, w.a, L.w_qkv, L.b_qkv, EAVQA_ACT_NONE, w.qkv, nullptr))) return rc;
        if ((rc = attn(b, w, l))) return rc;
        if ((rc = proj(b, w, l, O, E, E, w.ctx, L.w_o, L.b_o, EAVQA_ACT_NONE, w.x1, b.x))) return rc;
        if ((rc = eavqa_layernorm_fwd(b.dtype, 1, b.rows, E, w.x1, E, L.ln2_g, L.ln2_b, b.eps, w.a, E, nullptr, nullptr, b.stream))) return rc;
        if ((rc = proj(b, w, l, FC1, F, E, w.a, L.w_fc1, L.b_fc1, b.act, w.f, nullptr))) return rc;
        if ((rc = proj(b, w, l, FC2, E, F, w.f, L.w_fc2, L.b_fc2, EAVQA_ACT_NONE, b.x, w.x1))) return rc;
    }
    return EAVQA_OK;
}

// ---- splitk_loop policies.  norm: x = x_in + bias + sum(partials) (to x_out when non-null), LayerNorm(x) into the next product's operand.
// gemm: partial sums of A x W^T; A = nullptr: the operand norm() just left.
struct SplitK {             // bf16 weights: eavqa_layernorm_splitk into w.a, eavqa_gemm_splitk
    int norm(const Block& b, const LmWs& w, const float* x_in, const float* partials, int ks, const float* bias, float* x_out, const float* g,
             const float* beta) const {
        return eavqa_layernorm_splitk(b.dtype, b.rows, b.E, x_in, b.E, partials, ks, bias, x_out, x_out ? b.E : 0, g, beta, b.eps, w.a, b.E, b.stream);
    }
    int gemm(const Block& b, const LmWs& w, int, Proj, int N, int K, const void* A, const void* W, float* partials, int ks) const {
        return eavqa_gemm_splitk(b.dtype, b.rows, N, K, A ? A : w.a, K, W, K, partials, ks, b.stream);
    }
};
struct SplitKFp8 {          // e4m3 weights: the LayerNorm pass emits the quantised operand itself, other operands take the row quantiser
    const eavqa_lm_layer_scales_t* scales;
    int norm(const Block& b, const LmWs& w, const float* x_in, const float* partials, int ks, const float* bias, float* x_out, const float* g,
             const float* beta) const {
        return eavqa_layernorm_splitk_fp8(b.rows, b.E, x_in, b.E, partials, ks, bias, x_out, x_out ? b.E : 0, g, beta, b.eps, w.aq, b.E, w.asc, b.stream);
    }
    int gemm(const Block& b, const LmWs& w, int l, Proj p, int N, int K, const void* A, const void* W, float* partials, int ks) const {
        if (A)
            if (int rc = eavqa_quantize_rows_fp8(b.dtype, b.rows, K, A, K, w.aq, K, w.asc, b.stream)) return rc;
        return eavqa_gemm_fp8_splitk(b.rows, N, K, w.aq, K, w.asc, W, K, scale_of(scales[l], p), partials, ks, b.stream);
    }
};

// One decode step: split-K weight streaming; every GEMM leaves fp32 partial sums that its consumer adds up.
template <class P> int splitk_loop(const Block& b, const LmWs& w, const P& p, bool attn_from_partials, int row0, int S_max) {
    const int E = b.E, F = b.F, rows = b.rows, dtype = b.dtype;
    const SplitPlan& d = w.plan;
    int rc;
    for (int l = 0; l < b.n_layer; ++l) {
        const eavqa_lm_layer_t& L = b.layers[l];
        // x = x1 + b_fc2 + sum(FFN-down partials of the previous layer); operand = LN1(x)
        if (l == 0) rc = p.norm(b, w, b.x, nullptr, 0, nullptr, nullptr, L.ln1_g, L.ln1_b);
        else rc = p.norm(b, w, w.x1, w.down, d.fc2, b.layers[l - 1].b_fc2, b.x, L.ln1_g, L.ln1_b);
        if (rc) return rc;
        if ((rc = p.gemm(b, w, l, QKV, 3 * E, E, nullptr, L.w_qkv, w.part, d.qkv))) return rc;
        if (attn_from_partials) {
            // the decode attention sums the QKV partial sums itself (q, and the new K / V rows, which it appends to the cache)
            if ((rc = eavqa_attention_decode_splitk(dtype, b.B, b.H, row0 + 1, b.hd(), w.part, d.qkv, L.b_qkv, L.k_cache, E, L.v_cache, E, S_max, w.ctx, E,
                                                    b.key_mask, b.ld_mask, b.scale(), b.stream))) return rc;
        } else {
            // q -> qkv[:, :E]; k, v -> cache rows (sample m at row m * S_max + row0)
            if ((rc = eavqa_splitk_finish(dtype, rows, 3 * E, w.part, d.qkv, L.b_qkv, EAVQA_ACT_NONE, nullptr, 0, 0, 3, w.qkv, 3 * E,
                                          static_cast<char*>(L.k_cache) + (size_t)row0 * E * b.es(), (int64_t)S_max * E,
                                          static_cast<char*>(L.v_cache) + (size_t)row0 * E * b.es(), (int64_t)S_max * E, b.stream))) return rc;
            if ((rc = eavqa_attention_fwd(dtype, b.B, b.H, 1, row0 + 1, b.hd(), w.qkv, 3 * E, L.k_cache, E, L.v_cache, E, w.ctx, E, 1, S_max, b.key_mask,
                                          b.ld_mask, nullptr, 1, b.scale(), nullptr, b.stream))) return rc;
        }
        if ((rc = p.gemm(b, w, l, O, E, E, w.ctx, L.w_o, w.part, d.o))) return rc;
        // x1 = x + b_o + sum(partials); operand = LN2(x1)
        if ((rc = p.norm(b, w, b.x, w.part, d.o, L.b_o, w.x1, L.ln2_g, L.ln2_b))) return rc;
        if ((rc = p.gemm(b, w, l, FC1, F, E, nullptr, L.w_fc1, w.part, d.fc1))) return rc;
        if ((rc = eavqa_splitk_finish(dtype, rows, F, w.part, d.fc1, L.b_fc1, b.act, nullptr, 0, 0, 1, w.f, F, nullptr, 0, nullptr, 0, b.stream))) return rc;
        if ((rc = p.gemm(b, w, l, FC2, E, F, w.f, L.w_fc2, w.down, d.fc2))) return rc;
    }
    // x = x1 + b_fc2 + sum(last FFN-down partials)
    return eavqa_splitk_finish(dtype, rows, E, w.down, d.fc2, b.layers[b.n_layer - 1].b_fc2, EAVQA_ACT_NONE, w.x1, E, 1, 1, b.x, E, nullptr, 0, nullptr, 0,
                               b.stream);
}
}

extern "C" int64_t eavqa_lm_block_workspace_bytes(int dtype, int rows, int E, int F) { return lm_bytes(Family::Forward, dtype, rows, E, F); }

extern "C" int eavqa_lm_block_forward(int dtype, int n_layer, const eavqa_lm_layer_t* layers, int E, int H, int F, int act,
                                      float eps, int B, int Sq, int row0, int S_max, float* x, const int32_t* key_mask,
                                      int64_t ld_mask, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!layers || !x || !workspace || n_layer <= 0 || B <= 0 || Sq <= 0 || row0 < 0 || S_max < row0 + Sq) return EAVQA_E_ARG;
    if (E % H) return EAVQA_E_SHAPE;
    const int rows = B * Sq;
    Arena arena(workspace);
    const LmWs w = lm_layout(arena, Family::Forward, dtype, rows, E, F);
    if (workspace_bytes < (int64_t)arena.used) return EAVQA_E_ARG;
    const Block b{dtype, n_layer, layers, E, H, F, act, eps, B, rows, x, key_mask, ld_mask, stream};
    // A decode step takes the split-K route whenever it has a plan.  Tried and dropped (round 2): QKV and FFN-up through eavqa_gemm's M <= 64
    // tile kernels with fused epilogues and an appending attention, 7 kernels per layer instead of 9 - 3.42 against 3.16 ms per step (OPT-2.7B,
    // B = 32): with weights cold from HBM ~100 tile workgroups keep too few bytes in flight, split-K spreads a product over 500+.
    if (Sq == 1 && w.plan.ok) return splitk_loop(b, w, SplitK{}, attends_from_partials(E / H, row0 + 1, E), row0, S_max);
    return plain_loop(b, w, Gemm{0}, AppendAttn{Sq, row0, S_max});
}

// ------------------------------------------------------------------------------------------------ G rows per prompt over one prompt cache
// One new position of B * G rows (beams / draws of B prompts): plain_loop with eavqa_attention_decode_shared in place of "append +
// attention".  B * G is usually above the 64 rows of the split-K decode route, so the projections go through eavqa_gemm; only the QKV
// product of a step of <= 64 bf16 rows takes the split-K kernel + finish pass, so that q and the appended K / V rows are bit for bit what
// eavqa_lm_block_forward computes for the same rows (its decode route sums the same partial sums in the same order).
extern "C" int64_t eavqa_lm_block_step_shared_workspace_bytes(int dtype, int rows, int E, int F) {
    return lm_bytes(Family::Shared, dtype, rows, E, F);
}

extern "C" int eavqa_lm_block_step_shared(int dtype, int n_layer, const eavqa_lm_layer_t* layers, const eavqa_lm_tail_t* tails, int E, int H,
                                          int F, int act, float eps, int B, int G, int S0, int S_max, int t, int t_max, float* x,
                                          const int32_t* key_mask, int64_t ld_mask, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!layers || !tails || !x || !workspace || n_layer <= 0 || B <= 0 || H <= 0 || E <= 0 || F <= 0 || S_max < S0 || t < 0 || t >= t_max)
        return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (E % H) return EAVQA_E_SHAPE;
    const int hd = E / H, rows = B * G;
    if (G < 1 || G > 8 || hd % 8 || hd > 128 || S0 < 1 || S0 > 3584 || t_max > 256) return EAVQA_E_SHAPE;
    for (int l = 0; l < n_layer; ++l)
        if (!layers[l].k_cache || !layers[l].v_cache || !tails[l].k_tail || !tails[l].v_tail) return EAVQA_E_ARG;
    Arena arena(workspace);
    const LmWs w = lm_layout(arena, Family::Shared, dtype, rows, E, F);
    if (workspace_bytes < (int64_t)arena.used) return EAVQA_E_ARG;
    const Block b{dtype, n_layer, layers, E, H, F, act, eps, B, rows, x, key_mask, ld_mask, stream};
    return plain_loop(b, w, Gemm{w.plan.qkv}, SharedAttn{tails, G, S0, S_max, t, t_max});
}

// ------------------------------------------------------------------------------------------------ frozen LM held in e4m3 (BASELINE configs[4])
// The same driver for weights in e4m3 (models/lm.py Fp8Weight: bytes + one scale per tensor).  Every Linear is what the training / re-forward
// path computes - rows quantised to e4m3 with their own scale (eavqa_quantize_rows_fp8), product on the fp8 matrix cores, scales in the
// epilogue - so a cached generation reproduces `use_cache=False` (the reference's own loop, src/models/clipcap.py:414-419, through
// eavqa_gemm_fp8) up to fp32 summation order.  Decode steps stream HALF the weight bytes of the bf16 step: split-K over e4m3 weights
// (eavqa_gemm_fp8_splitk), the LayerNorm pass emits the quantised operand of the next projection itself (eavqa_layernorm_splitk_fp8); the
// attention output and the FFN activation take the stand-alone row quantiser (two more short kernels per layer).
extern "C" int64_t eavqa_lm_block_fp8_workspace_bytes(int rows, int E, int F) { return lm_bytes(Family::Fp8, EAVQA_BF16, rows, E, F); }

extern "C" int eavqa_lm_block_forward_fp8(int n_layer, const eavqa_lm_layer_t* layers, const eavqa_lm_layer_scales_t* scales, int E, int H, int F, int act,
                                          float eps, int B, int Sq, int row0, int S_max, float* x, const int32_t* key_mask, int64_t ld_mask,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
    if (!layers || !scales || !x || !workspace || n_layer <= 0 || B <= 0 || Sq <= 0 || row0 < 0 || S_max < row0 + Sq) return EAVQA_E_ARG;
    if (E % H || E % 128 || F % 128) return EAVQA_E_SHAPE;                            // eavqa_gemm_fp8: K % 128
    const int rows = B * Sq;
    Arena arena(workspace);
    const LmWs w = lm_layout(arena, Family::Fp8, EAVQA_BF16, rows, E, F);
    if (workspace_bytes < (int64_t)arena.used) return EAVQA_E_ARG;
    const Block b{EAVQA_BF16, n_layer, layers, E, H, F, act, eps, B, rows, x, key_mask, ld_mask, stream};
    if (Sq == 1 && w.plan.ok && attends_from_partials(E / H, row0 + 1, E)) return splitk_loop(b, w, SplitKFp8{scales}, true, row0, S_max);
    return plain_loop(b, w, GemmFp8{scales}, AppendAttn{Sq, row0, S_max});        // prefill, or a shape without a plan
}
