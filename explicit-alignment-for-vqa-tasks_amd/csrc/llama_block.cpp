// Host-side driver: all decoder layers of a frozen Llama-family LM in ONE C call (eavqa_llama_block_forward in include/eavqa_llama.h) - the
// counterpart of eavqa_lm_block_forward (lm_block.cpp) for pre-RMSNorm layers with rotary positions, a SwiGLU feed-forward and no
// biases, composed from the public entry points in the same way.  Prefill: Sq = prompt length, row0 = 0; cached step: Sq = 1.  Pure
// enqueue: no allocation (the caller passes a workspace), no synchronisation, graph-capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "block_ws.h"
#include "eavqa.h"
#include "eavqa_llama.h"

namespace {
using eavqa_block::Arena;

// Split counts of a decode step's four products and its two partial-sum regions in floats: `scratch` serves QKV, out-projection and
// gate | up in turn, `down` holds the down-projection's partial sums until the next layer's RMSNorm adds them up.  The step takes the
// split-K route when the three products with K = E have a plan; a down-projection without one (down = 0: K = F has no slice count that
// fits, e.g. 11008 at 32 rows) goes through eavqa_gemm with the residual in its epilogue and leaves no partial sums.
struct SplitPlan { int qkv, o, gu, down; bool ok; size_t scratch, down_floats; };
inline SplitPlan plan_split(int dtype, int rows, int E, int F) {
    SplitPlan d{};
    if (dtype != EAVQA_BF16 || rows > 64 || E % 8 || F % 4) return d;
    d.qkv = eavqa_gemm_splitk_plan(rows, 3 * E, E), d.o = eavqa_gemm_splitk_plan(rows, E, E);
    d.gu = eavqa_gemm_splitk_plan(rows, 2 * F, E), d.down = eavqa_gemm_splitk_plan(rows, E, F);
    d.ok = d.qkv > 0 && d.o > 0 && d.gu > 0;
    if (d.down < 0) d.down = 0;
    const size_t a = (size_t)d.qkv * 3 * E, b = (size_t)d.o * E, c = (size_t)d.gu * 2 * F;
    d.scratch = (a > b ? (a > c ? a : c) : (b > c ? b : c)) * rows;
    d.down_floats = (size_t)d.down * rows * E;
    return d;
}

// ONE layout: the size function and the driver both run it, and the partial sums are sized from the plan the step itself uses.
struct Ws { void* a; char* qkv; void* ctx; float* x1; void* u; void* h; SplitPlan plan; float* part; float* down; };
inline Ws layout(Arena& A, int dtype, int rows, int E, int F) {
    const size_t es = dtype == EAVQA_BF16 ? 2 : 4, R = rows;
    Ws w{};
    w.a = A.take(R * E * es);                   // RMSNorm output
    w.qkv = A.take<char>(R * 3 * E * es);       // q | k | v, q and k rotated
    w.ctx = A.take(R * E * es);                 // attention output
    w.x1 = A.take<float>(R * E * 4);            // fp32 residual stream behind the attention block
    w.u = A.take(R * 2 * F * es);               // gate | up
    w.h = A.take(R * F * es);                   // silu(gate) * up
    w.plan = plan_split(dtype, rows, E, F);
    if (w.plan.ok) {
        w.part = A.take<float>(w.plan.scratch * 4);
        if (w.plan.down) w.down = A.take<float>(w.plan.down_floats * 4);
    }
    return w;
}

struct Block {
    int dtype, n_layer; const eavqa_llama_layer_t* layers; int E, H, F; float eps; int B, rows; float* x; const int32_t* pos; const float* cos;
    const float* sin; int n_pos; const int32_t* key_mask; int64_t ld_mask; void* stream;
    int hd() const { return E / H; }
    float scale() const { return 1.0f / sqrtf((float)hd()); }
    size_t es() const { return dtype == EAVQA_BF16 ? 2 : 4; }
};

// C [rows, N] = A [rows, K] x W^T (+ res): with a residual C is the fp32 stream
inline int gemm(const Block& b, int N, int K, const void* A, const void* W, void* C, const float* res) {
    return eavqa_gemm(b.dtype, 1, 1, b.rows, N, K, A, K, W, K, C, N, res || b.dtype == EAVQA_F32, 1.f, nullptr, EAVQA_ACT_NONE, nullptr, nullptr, 0, res,
                      res ? N : 0, b.stream);
}

int plain_loop(const Block& b, const Ws& w, int Sq, int row0, int S_max) {
    const int E = b.E, F = b.F, hd = b.hd();
    int rc;
    for (int l = 0; l < b.n_layer; ++l) {
        const eavqa_llama_layer_t& L = b.layers[l];
        if ((rc = eavqa_rmsnorm_fwd(b.dtype, 1, b.rows, E, b.x, E, L.ln1_g, b.eps, w.a, E, nullptr, b.stream))) return rc;
        if ((rc = gemm(b, 3 * E, E, w.a, L.w_qkv, w.qkv, nullptr))) return rc;
        // q and k are the first 2 E columns: one call over 2 H heads
        if ((rc = eavqa_rope(b.dtype, b.rows, 2 * b.H, hd, w.qkv, 3 * E, b.pos, b.cos, b.sin, hd / 2, b.n_pos, 0, b.stream))) return rc;
        if ((rc = eavqa_copy_rows(b.dtype, b.B, Sq, E, w.qkv + (size_t)E * b.es(), 3 * E, Sq, L.k_cache, E, S_max, row0, b.stream))) return rc;
        if ((rc = eavqa_copy_rows(b.dtype, b.B, Sq, E, w.qkv + (size_t)2 * E * b.es(), 3 * E, Sq, L.v_cache, E, S_max, row0, b.stream))) return rc;
        if ((rc = eavqa_attention_fwd(b.dtype, b.B, b.H, Sq, row0 + Sq, hd, w.qkv, 3 * E, L.k_cache, E, L.v_cache, E, w.ctx, E, Sq, S_max, b.key_mask,
                                      b.ld_mask, nullptr, 1, b.scale(), nullptr, b.stream))) return rc;
        if ((rc = gemm(b, E, E, w.ctx, L.w_o, w.x1, b.x))) return rc;
        if ((rc = eavqa_rmsnorm_fwd(b.dtype, 1, b.rows, E, w.x1, E, L.ln2_g, b.eps, w.a, E, nullptr, b.stream))) return rc;
        if ((rc = gemm(b, 2 * F, E, w.a, L.w_gu, w.u, nullptr))) return rc;
        if ((rc = eavqa_swiglu_fwd(b.dtype, b.rows, F, w.u, 2 * F, w.h, F, b.stream))) return rc;
        if ((rc = gemm(b, E, F, w.h, L.w_down, b.x, w.x1))) return rc;
    }
    return EAVQA_OK;
}

// One decode step: split-K weight streaming; every product leaves fp32 partial sums that its consumer adds up.
int splitk_loop(const Block& b, const Ws& w, int row0, int S_max) {
    const int E = b.E, F = b.F, rows = b.rows, dtype = b.dtype, hd = b.hd();
    const SplitPlan& d = w.plan;
    int rc;
    for (int l = 0; l < b.n_layer; ++l) {
        const eavqa_llama_layer_t& L = b.layers[l];
        // x = x1 + sum(down partials of the previous layer); operand = RMSNorm(x)
        if (l == 0 || !d.down) rc = eavqa_rmsnorm_splitk(dtype, rows, E, b.x, E, nullptr, 0, nullptr, 0, L.ln1_g, b.eps, w.a, E, b.stream);
        else rc = eavqa_rmsnorm_splitk(dtype, rows, E, w.x1, E, w.down, d.down, b.x, E, L.ln1_g, b.eps, w.a, E, b.stream);
        if (rc) return rc;
        if ((rc = eavqa_gemm_splitk(dtype, rows, 3 * E, E, w.a, E, L.w_qkv, E, w.part, d.qkv, b.stream))) return rc;
        if ((rc = eavqa_rope_finish(dtype, rows, b.H, hd, w.part, d.qkv, b.pos, b.cos, b.sin, hd / 2, b.n_pos, w.qkv, 3 * E, b.stream))) return rc;
        // the attention appends the rotated k and v of the new position to the cache itself
        if ((rc = eavqa_attention_decode(dtype, b.B, b.H, row0 + 1, hd, w.qkv, 3 * E, L.k_cache, E, L.v_cache, E, S_max, w.qkv + (size_t)E * b.es(),
                                         w.qkv + (size_t)2 * E * b.es(), 3 * E, w.ctx, E, b.key_mask, b.ld_mask, b.scale(), b.stream))) return rc;
        if ((rc = eavqa_gemm_splitk(dtype, rows, E, E, w.ctx, E, L.w_o, E, w.part, d.o, b.stream))) return rc;
        // x1 = x + sum(partials); operand = RMSNorm(x1)
        if ((rc = eavqa_rmsnorm_splitk(dtype, rows, E, b.x, E, w.part, d.o, w.x1, E, L.ln2_g, b.eps, w.a, E, b.stream))) return rc;
        if ((rc = eavqa_gemm_splitk(dtype, rows, 2 * F, E, w.a, E, L.w_gu, E, w.part, d.gu, b.stream))) return rc;
        if ((rc = eavqa_swiglu_splitk(dtype, rows, F, w.part, d.gu, w.h, F, b.stream))) return rc;
        if (d.down) rc = eavqa_gemm_splitk(dtype, rows, E, F, w.h, F, L.w_down, F, w.down, d.down, b.stream);
        else rc = gemm(b, E, F, w.h, L.w_down, b.x, w.x1);         // x = x1 + h W^T
        if (rc) return rc;
    }
    if (!d.down) return EAVQA_OK;
    // x = x1 + sum(last down partials)
    return eavqa_splitk_finish(dtype, rows, E, w.down, d.down, nullptr, EAVQA_ACT_NONE, w.x1, E, 1, 1, b.x, E, nullptr, 0, nullptr, 0, b.stream);
}
}

extern "C" int64_t eavqa_llama_block_workspace_bytes(int dtype, int rows, int E, int F) {
    if (rows <= 0 || E <= 0 || F <= 0) return 0;
    Arena count(nullptr);
    layout(count, dtype, rows, E, F);
    return (int64_t)count.used;
}

extern "C" int eavqa_llama_block_forward(int dtype, int n_layer, const eavqa_llama_layer_t* layers, int E, int H, int F, float eps, int B, int Sq,
                                         int row0, int S_max, float* x, const int32_t* pos, const float* cos, const float* sin, int n_pos,
                                         const int32_t* key_mask, int64_t ld_mask, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!layers || !x || !pos || !cos || !sin || !workspace || n_layer <= 0 || B <= 0 || Sq <= 0 || row0 < 0 || S_max < row0 + Sq || n_pos <= 0)
        return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (E <= 0 || H <= 0 || F <= 0 || E % H || (E / H) % 8 || E / H > 256 || (int64_t)B * Sq > (int64_t)1 << 24) return EAVQA_E_SHAPE;
    const int rows = B * Sq, hd = E / H;
    Arena arena(workspace);
    const Ws w = layout(arena, dtype, rows, E, F);
    if (workspace_bytes < (int64_t)arena.used) return EAVQA_E_ARG;
    const Block b{dtype, n_layer, layers, E, H, F, eps, B, rows, x, pos, cos, sin, n_pos, key_mask, ld_mask, stream};
    // eavqa_attention_decode: hd <= 128 and at most 3584 keys
    if (Sq == 1 && w.plan.ok && hd <= 128 && row0 + 1 <= 3584) return splitk_loop(b, w, row0, S_max);
    return plain_loop(b, w, Sq, row0, S_max);
}
