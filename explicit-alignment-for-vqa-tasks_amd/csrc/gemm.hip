// MFMA GEMM with fused epilogue for gfx950 (eavqa_gemm in include/eavqa.h).
//
//   C[M,N] = epilogue(alpha * sum_k A(m,k) * B(n,k))
//
// Two kernels share one tile shape (128x128 output per 256-thread workgroup, 2x2 waves,
// 64x64 per wave) and one LDS-staged epilogue:
//   * bf16: v_mfma_f32_16x16x32_bf16, BK = 64, operands staged k-contiguous in LDS as
//     [128 rows][64 k] with a 16-byte-chunk XOR swizzle (chunk ^= row & 7) so that the
//     ds_read_b128 fragment reads are bank-conflict free;
//   * f32 : v_mfma_f32_32x32x2_f32 (exact fp32 fmaf chain - the parity path), BK = 16,
//     operands staged as [128 rows][16 k] with a 17-float row pitch.
// Global->LDS staging goes through registers: the loads of K-tile t+1 are issued before
// the MFMAs of tile t and written to the other LDS buffer after them (one barrier per tile).
// An operand whose contiguous memory dimension is NOT k (Conv1D-style [K,N] weights, the
// transposed operands of the mapper's dgrad/wgrad) is transposed while it is written to LDS.
// The accumulators leave through LDS so that bias / residual / aux traffic and the C stores
// are 16-byte row-contiguous accesses.
#include "common.h"

namespace {

// Kernel-selection knobs of eavqa_gemm_ex (include/eavqa_test.h), decoded per call: the library keeps no mutable state.
struct Knobs {
    int stagger;        // [3:0]   s_sleep units for odd co-resident blocks of the round-1 128 x 128 kernel (experiment)
    int ablate;         // [6:4]   timing-only ablation variant of that kernel (results wrong when non-zero)
    bool disable_fast;  // [7]     general register-staged kernel on fast-path shapes (parity coverage of that kernel)
    int k64_mode;       // [13:8]  full-line (BK = 64) family: 0 = by cost model, 1 = never (round-1 dispatch), 2.. force K64_SHAPES[id - 2]
    int big_mode;       // [15:14] round-1 256 x 256 kernel: 0 by shape, 1 never, 2 always (K % 64 == 0)
    int deep;           // [17:16] 2 = force the 8-stage ring of the round-1 128 x 128 kernel (experiment)
    int shape_mode;     // [20:18] round-1 shaped tiles: 0 by cost model, 1 never, 2.. force SHAPES[id - 2]
    int group_n;        // [24:21] 256 x 256 kernel, tile order inside an XCD: 0 = library default, 1 = m fastest (round 2), 2.. = groups of (value - 1) columns
    bool no_row_split;  // [25]    256 x 256 kernel: keep a ragged last tile row in the same launch (A / B of big_split_rows)
    explicit Knobs(int k = 0) : stagger(k & 15), ablate((k >> 4) & 7), disable_fast(((k >> 7) & 1) != 0), k64_mode((k >> 8) & 63),
                                big_mode((k >> 14) & 3), deep((k >> 16) & 3), shape_mode((k >> 18) & 7), group_n((k >> 21) & 15),
                                no_row_split(((k >> 25) & 1) != 0) {}
};

// GemmParamsBase is the kernel argument of the plain kernels; GemmParams (below) adds the eavqa_gemm_ln fields and is what the host code and the
// LN instantiations pass: the plain launches carry the kernel arguments they always did (88 bytes - two cache lines - fewer than the full struct).
struct GemmParamsBase {
    const void* A; const void* B; void* C;
    const float* bias; const void* aux_in; void* aux_out; const void* residual;   // residual: float32, or the operand dtype when res_lowp
    const float* row_scale;        // fp8 path: per-row dequantisation scale of A (multiplies alpha), else NULL
    int M, N, K;
    int64_t lda, ldb, ldc, ld_aux, ldr;
    int act, out_f32, res_lowp;   // res_lowp: 0 float32 residual, 1 operand dtype, 2 half
    int out_f16;                  // C (when not float32) is half instead of the operand dtype
    int ablate;                    // eavqa_gemm_ex timing-only ablations of the specialised kernels (0 in the product path)
    float alpha;
    int tiles_m, tiles_n;
    int group_n;                   // 256 x 256 kernel: tile columns per group of the in-XCD tile order (0 = m fastest)
    int vec_c, vec_aux, vec_res, vec_bias;   // 16-byte (8-byte for bf16) vector access allowed on C / aux / residual / bias
};
struct GemmParams : GemmParamsBase {
    // -- eavqa_gemm_ln (LayerNorm of a frozen LM folded into its neighbours, include/eavqa.h) --
    // producer side: a second copy of the result in the operand dtype and (sum, sum of squares) of every result row per 64-column slot
    void* copy_out = nullptr; int64_t ld_copy = 0; int vec_copy = 0;
    float* stats_out = nullptr; int stats_ld = 0;          // [M][stats_ld][2]; slots a tile does not own are written as zeros by the last tile column
    // consumer side: A holds UN-normalised rows x; B holds W * gamma; C = rstd (alpha acc - mean c) + bias with (mean, rstd) from the row sums
    const float* ln_stats = nullptr; int ln_parts = 0, ln_ld = 0;
    const float* ln_c = nullptr; float ln_inv_n = 0.f, ln_eps = 0.f;
    float* mean_out = nullptr; float* rstd_out = nullptr;  // [M], written by the tiles of column 0 (LayerNorm backward reads them)
    // -- eavqa_gemm_pf: the weight matrix the next GEMM in program order will stream (csrc/gemm_k64.hip, "Look-ahead"); null / 0 = nothing to do --
    const void* pf_ptr = nullptr; int64_t pf_bytes = 0;
};
// kernel argument of the eavqa_gemm_pf instantiations: the plain one plus the region
struct GemmParamsPf : GemmParamsBase { const void* pf_ptr; int64_t pf_bytes; };
constexpr int LN_ROWSTAT_BYTES = 2048;                 // (rstd, -rstd mean) of up to 256 tile rows, behind a kernel's ring / C tile in dynamic LDS
inline int ln_lds(const GemmParams& p) { return p.ln_stats ? LN_ROWSTAT_BYTES : 0; }
// kernel-side view: the full struct from either kernel argument (the LN fields of a plain launch are compile-time nulls: their code folds away)
__device__ __forceinline__ GemmParams widen(const GemmParams& k) { return k; }
__device__ __forceinline__ GemmParams widen(const GemmParamsBase& k) { GemmParams p; static_cast<GemmParamsBase&>(p) = k; return p; }
__device__ __forceinline__ GemmParams widen(const GemmParamsPf& k) { GemmParams p = widen(static_cast<const GemmParamsBase&>(k)); p.pf_ptr = k.pf_ptr; p.pf_bytes = k.pf_bytes; return p; }
template <bool LNX> struct KernArg { using type = GemmParamsBase; };
template <> struct KernArg<true> { using type = GemmParams; };

constexpr int BM = 128, BN = 128;
constexpr int CS_PITCH = 132;                       // floats per row of the staged C tile
constexpr int CS_BYTES = BM * CS_PITCH * 4;         // 67,584 B

// XCD-aware, bijective block -> tile map: the dispatcher deals blocks round-robin over the
// 8 XCDs, so give each XCD a contiguous run of tiles (M fastest) to share operand panels in L2.
__device__ __forceinline__ void tile_coords(const GemmParams& p, int& tm, int& tn) {
    const int nwg = p.tiles_m * p.tiles_n;
    const int bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    tm = wgid % p.tiles_m;
    tn = wgid / p.tiles_m;
}

// eavqa_gemm_ln, consumer side: (rstd, -rstd mean) of the tile's rows from the producer's partial sums, once per tile.  Any subset of the
// workgroup's threads may run it (tid in [0, nthreads)); a barrier lies between it and the epilogue in every kernel.
__device__ __forceinline__ void ln_rowstat_fill(const GemmParams& p, float2* rowstat, int m0, int n0, int rows, int tid, int nthreads) {
    if (!p.ln_stats) return;
    for (int r = tid; r < rows; r += nthreads) {
        const int m = min(m0 + r, p.M - 1);
        const float2* q = reinterpret_cast<const float2*>(p.ln_stats) + (int64_t)m * p.ln_ld;
        float s = 0.f, ss = 0.f;
        if (((p.ln_ld | p.ln_parts) & 1) == 0 && (reinterpret_cast<uintptr_t>(p.ln_stats) & 15) == 0) {
            // two slots per 16-byte load, four loads in flight (a row's slots are contiguous); slots past the end are re-read from the last
            // pair and multiplied by zero, so the order of the additions does not depend on the slot count's remainder
            const float4* q4 = reinterpret_cast<const float4*>(q);
            const int n4 = p.ln_parts >> 1;
            for (int i = 0; i < n4; i += 4) {
                float4 t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) t[k] = q4[min(i + k, n4 - 1)];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float w = (i + k < n4) ? 1.f : 0.f;
                    s += w * (t[k].x + t[k].z);
                    ss += w * (t[k].y + t[k].w);
                }
            }
        } else {
            for (int i = 0; i < p.ln_parts; ++i) { const float2 t = q[i]; s += t.x; ss += t.y; }
        }
        const float mean = s * p.ln_inv_n;
        const float rstd = 1.0f / sqrtf(fmaxf(ss * p.ln_inv_n - mean * mean, 0.f) + p.ln_eps);
        rowstat[r] = make_float2(rstd, -rstd * mean);
        if (n0 == 0 && m0 + r < p.M && p.mean_out) { p.mean_out[m] = mean; p.rstd_out[m] = rstd; }
    }
}

// ---- epilogue shared by all kernels: Cs holds the 128x128 fp32 tile (pitch CS_PITCH) ----
// MODE: 0 = no activation, 1 = forward activation, 2 = multiply by the activation derivative at aux_in.
// FULL: the tile lies entirely inside C and every operand allows vector access: no bounds checks, 8/16-byte
// accesses only (every tile of the hot shapes except the last row of tiles).
// Geometry G: TPR threads cover one row of the staged tile (4 columns each), RPP rows per pass, NPASS passes, PITCH floats
// per staged row.
// ROWS < RPP * NPASS (tile widths that do not divide the block): threads beyond TPR * RPP idle, the last pass is cut at ROWS.
template <int TPR_, int RPP_, int NPASS_, int PITCH_, int ROWS_ = RPP_ * NPASS_, int LN_UNROLL_ = 4> struct EpiGeo {
    static constexpr int TPR = TPR_, RPP = RPP_, NPASS = NPASS_, PITCH = PITCH_, ROWS = ROWS_;
    static constexpr int LN_UNROLL = LN_UNROLL_;      // passes in flight in the eavqa_gemm_ln form of the epilogue (1 where registers are short)
};
using EpiGeo128 = EpiGeo<32, 8, 16, CS_PITCH>;      // 128 x 128 tile, 256 threads

// one row m, four consecutive columns n .. n + 3: v[] = the fp32 accumulators on entry
template <typename T, int ACT, int MODE, bool FULL, bool LNX>
__device__ __forceinline__ void epilogue_quad(const GemmParams& p, int m, int n, float (&v)[4], const float (&bias4)[4], const float2 rs,
                                              const float (&c4)[4]) {
    const T* aux_in = reinterpret_cast<const T*>(p.aux_in);
    T* aux_out = reinterpret_cast<T*>(p.aux_out);
    const bool full = FULL || (n + 3 < p.N);
    const float al = p.row_scale ? p.alpha * p.row_scale[m] : p.alpha;
    if (LNX && p.ln_stats) {                             // rstd (alpha acc - mean c[n]) + bias[n]
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (al * rs.x) * v[j] + (bias4[j] + rs.y * c4[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = al * v[j] + bias4[j];
    }
    if (aux_out) {
        T* q = aux_out + (int64_t)m * p.ld_aux + n;
        if (FULL || (full && p.vec_aux)) elem<T>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<T>::st(q + j, v[j]);
    }
    if (MODE == 2) {
        const T* q = aux_in + (int64_t)m * p.ld_aux + n;
        float u[4] = {0.f, 0.f, 0.f, 0.f};
        if (FULL || (full && p.vec_aux)) { float4 t = elem<T>::ld4(q); u[0] = t.x; u[1] = t.y; u[2] = t.z; u[3] = t.w; }
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) u[j] = elem<T>::ld(q + j);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= act_bwd(ACT, u[j]);
    } else if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_fwd(ACT, v[j]);
    }
    if (p.residual) {
        if (p.res_lowp == 2) {                             // 16-bit residual stream of a frozen tower (the CLIP tower): half ...
            const f16_t* q = reinterpret_cast<const f16_t*>(p.residual) + (int64_t)m * p.ldr + n;
            if (FULL || (full && p.vec_res)) { float4 t = elem<f16_t>::ld4(q); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            else
                for (int j = 0; j < 4; ++j)
                    if (n + j < p.N) v[j] += elem<f16_t>::ld(q + j);
        } else if (p.res_lowp) {                           // ... or the operand dtype
            const T* q = reinterpret_cast<const T*>(p.residual) + (int64_t)m * p.ldr + n;
            if (FULL || (full && p.vec_res)) { float4 t = elem<T>::ld4(q); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            else
                for (int j = 0; j < 4; ++j)
                    if (n + j < p.N) v[j] += elem<T>::ld(q + j);
        } else {
            const float* q = reinterpret_cast<const float*>(p.residual) + (int64_t)m * p.ldr + n;
            if (FULL || (full && p.vec_res)) { float4 t = *reinterpret_cast<const float4*>(q); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            else
                for (int j = 0; j < 4; ++j)
                    if (n + j < p.N) v[j] += q[j];
        }
    }
    if (p.out_f32) {
        float* q = reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n;
        if (FULL || (full && p.vec_c)) *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) q[j] = v[j];
    } else if (p.out_f16) {
        f16_t* q = reinterpret_cast<f16_t*>(p.C) + (int64_t)m * p.ldc + n;
        if (FULL || (full && p.vec_c)) elem<f16_t>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<f16_t>::st(q + j, v[j]);
    } else {
        T* q = reinterpret_cast<T*>(p.C) + (int64_t)m * p.ldc + n;
        if (FULL || (full && p.vec_c)) elem<T>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<T>::st(q + j, v[j]);
    }
    if (LNX && p.copy_out) {
        T* q = reinterpret_cast<T*>(p.copy_out) + (int64_t)m * p.ld_copy + n;
        if (full && p.vec_copy) elem<T>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<T>::st(q + j, v[j]);
    }
}

template <bool FULL>
__device__ __forceinline__ void load_bias4(const GemmParams& p, int n, float (&bias4)[4]) {
    bias4[0] = bias4[1] = bias4[2] = bias4[3] = 0.f;
    if (p.bias) {
        if (FULL) { const float4 b = *reinterpret_cast<const float4*>(p.bias + n); bias4[0] = b.x; bias4[1] = b.y; bias4[2] = b.z; bias4[3] = b.w; }
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) bias4[j] = p.bias[n + j];
        }
    }
}

// LnArgs: where the tile's row statistics lie (eavqa_gemm_ln consumer side) and which of them this staged slab starts at
struct LnArgs { const float2* rowstat; int row_base; };

template <typename T, int ACT, int MODE, bool FULL, typename G, bool LNX>
__device__ __forceinline__ void epilogue_body(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln) {
    const int tid = threadIdx.x;
    if (G::ROWS != G::RPP * G::NPASS && tid >= G::TPR * G::RPP) return;
    const int c4 = (tid % G::TPR) * 4;
    const int n = n0 + c4;
    float bias4[4], lc4[4] = {0.f, 0.f, 0.f, 0.f};
    load_bias4<FULL>(p, n, bias4);
    if (LNX && p.ln_stats) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (FULL || n + j < p.N) lc4[j] = p.ln_c[n + j];
    }
    auto one_pass = [&](int pass) {
        const int row = (tid / G::TPR) + pass * G::RPP;
        const int m = m0 + row;
        if (G::ROWS != G::RPP * G::NPASS && row >= G::ROWS) return;
        if (!FULL && (m >= p.M || n >= p.N)) return;
        const float4 a = *reinterpret_cast<const float4*>(&Cs[row * G::PITCH + c4]);
        float v[4] = {a.x, a.y, a.z, a.w};
        const float2 rs = (LNX && p.ln_stats) ? ln.rowstat[ln.row_base + row] : make_float2(1.f, 0.f);
        epilogue_quad<T, ACT, MODE, FULL, LNX>(p, m, n, v, bias4, rs, lc4);
        if (LNX && p.stats_out) {                           // the values as stored (before any rounding), zeros beyond column N, back into the staged tile
            if (!FULL) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j >= p.N) v[j] = 0.f;
            }
            *reinterpret_cast<float4*>(&Cs[row * G::PITCH + c4]) = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    if constexpr (LNX && G::LN_UNROLL == 1) {               // (a literal count: the pragma does not take a dependent expression reliably)
#pragma unroll 1
        for (int pass = 0; pass < G::NPASS; ++pass) one_pass(pass);
    } else {
#pragma unroll 4
        for (int pass = 0; pass < G::NPASS; ++pass) one_pass(pass);
    }
}

// eavqa_gemm_ln, producer side: (sum, sum of squares) of the finished rows of this slab, one thread per row in column order (a fixed
// summation order: bitwise reproducible), into the 64-column slots the tile covers - the whole sum in the first, zeros in the others -
// and zeros into the slots behind the last tile column, so that a consumer adds all stats_ld slots without knowing the tile width.
template <typename G>
__device__ __forceinline__ void epilogue_row_sums(const GemmParams& p, const float* Cs, int m0, int n0) {
    constexpr int COLS = G::TPR * 4;
    static_assert(COLS >= 64 && COLS % 4 == 0, "a tile covers at least one 64-column slot");
    __syncthreads();
    const int cols = min(COLS, p.N - n0);
    const int slot0 = n0 / 64, slot1 = (n0 + COLS < p.N) ? (n0 + COLS) / 64 : p.stats_ld;     // this tile owns slots [slot0, slot1)
    for (int r = threadIdx.x; r < G::ROWS; r += blockDim.x) {
        const int m = m0 + r;
        if (m >= p.M) continue;
        float s = 0.f, ss = 0.f;
        for (int c = 0; c < cols; c += 4) {
            const float4 t = *reinterpret_cast<const float4*>(&Cs[r * G::PITCH + c]);
            s += (t.x + t.y) + (t.z + t.w);
            ss += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
        }
        float2* q = reinterpret_cast<float2*>(p.stats_out) + (int64_t)m * p.stats_ld;
        q[slot0] = make_float2(s, ss);
        for (int i = slot0 + 1; i < slot1; ++i) q[i] = make_float2(0.f, 0.f);
    }
}

template <typename T, int ACT, int MODE, typename G, bool LNX>
__device__ __forceinline__ void epilogue_mode(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln) {
    constexpr int ROWS = G::ROWS, COLS = G::TPR * 4;
    const bool full_tile = (m0 + ROWS <= p.M) && (n0 + COLS <= p.N) && p.vec_c && (!(p.aux_in || p.aux_out) || p.vec_aux) &&
                           (!p.residual || p.vec_res) && (!p.bias || p.vec_bias);
    if (full_tile) epilogue_body<T, ACT, MODE, true, G, LNX>(p, Cs, m0, n0, ln);
    else epilogue_body<T, ACT, MODE, false, G, LNX>(p, Cs, m0, n0, ln);
    if (LNX && p.stats_out) epilogue_row_sums<G>(p, Cs, m0, n0);
}

// block-uniform dispatch on the (runtime) activation id / mode: each combination gets its own straight-line body
// LNX = false compiles the eavqa_gemm_ln paths out (the 1024-thread 256 x 256 kernel has 128 registers per lane: its plain form must not carry them)
template <typename T, typename G = EpiGeo128, bool LNX = true>
__device__ __forceinline__ void epilogue(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln = LnArgs{nullptr, 0}) {
    const int mode = p.aux_in ? 2 : (p.act != EAVQA_ACT_NONE ? 1 : 0);
    if (mode == 0) { epilogue_mode<T, EAVQA_ACT_NONE, 0, G, LNX>(p, Cs, m0, n0, ln); return; }
    switch (p.act) {
        case EAVQA_ACT_TANH:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_TANH, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_TANH, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        case EAVQA_ACT_RELU:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_RELU, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_RELU, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        case EAVQA_ACT_GELU_NEW:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_GELU_NEW, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_GELU_NEW, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        case EAVQA_ACT_QUICK_GELU:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_QUICK_GELU, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_QUICK_GELU, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        default:   // aux_in with act == none: derivative 1
            epilogue_mode<T, EAVQA_ACT_NONE, 0, G, LNX>(p, Cs, m0, n0, ln);
    }
}

// the call every kernel with registers to spare makes: the plain epilogue unless the launch carries eavqa_gemm_ln arguments (block-uniform)
template <typename T, typename G = EpiGeo128>
__device__ __forceinline__ void epilogue_any(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln = LnArgs{nullptr, 0}) {
    if (p.ln_stats || p.stats_out || p.copy_out) epilogue<T, G, true>(p, Cs, m0, n0, ln);
    else epilogue<T, G, false>(p, Cs, m0, n0, ln);
}

// (Round 3 built a direct register -> global epilogue for the specialised tiles - operands swapped, B fragment rows permuted so that a
// lane owns 16 consecutive columns - and measured it 10-70 % SLOWER than the LDS-staged pass below (a wave's store covers 16 rows x
// 32 bytes: partial lines); removed again, numbers in profiles/round3_direct_epilogue.md.)

// =============================================================== bf16 ===
constexpr int BK16 = 64;                          // k per LDS tile (bf16)
constexpr int OPER16_BYTES = 128 * BK16 * 2;      // 16 KiB per operand per buffer

// byte offset of the 16-byte chunk (row, kc) inside a swizzled [128][64] bf16 tile
__device__ __forceinline__ int swz16(int row, int kc) { return row * 128 + ((kc ^ (row & 7)) << 4); }

// Stage one operand tile (128 rows x 64 k) from global memory into registers.
// KC: memory is [rows][K] (k contiguous); else memory is [K][rows] (row contiguous).
template <bool KC>
__device__ __forceinline__ void g2r_16(uint4 (&r)[4], const bf16_t* X, int64_t ld, int row0, int rows_max,
                                       int k0, int K) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (KC) {
            const int row = c >> 3, kc = c & 7;
            const int gr = row0 + row, gk = k0 + kc * 8;
            if (gr < rows_max && gk < K) v = *reinterpret_cast<const uint4*>(X + (int64_t)gr * ld + gk);
        } else {
            const int k = c >> 4, rc = c & 15;
            const int gk = k0 + k, gr = row0 + rc * 8;
            if (gk < K && gr < rows_max) v = *reinterpret_cast<const uint4*>(X + (int64_t)gk * ld + gr);
        }
        r[i] = v;
    }
}
template <bool KC>
__device__ __forceinline__ void r2s_16(const uint4 (&r)[4], char* S) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i;
        if (KC) {
            const int row = c >> 3, kc = c & 7;
            *reinterpret_cast<uint4*>(S + swz16(row, kc)) = r[i];
        } else {
            const int k = c >> 4, rc = c & 15;
            const unsigned w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = rc * 8 + j;
                const unsigned short e = (unsigned short)((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu));
                *reinterpret_cast<unsigned short*>(S + swz16(row, k >> 3) + (k & 7) * 2) = e;
            }
        }
    }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS carve: A buffers at 0 / 16 KiB, B buffers at 32 / 48 KiB (pointer arrays of LDS addresses
    // would become static initialisers, which the backend rejects - use offsets)
    char* const As0 = smem;
    char* const Bs0 = smem + 2 * OPER16_BYTES;

    int tm, tn;
    tile_coords(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = (p.K + BK16 - 1) / BK16;
    uint4 ra[4], rb[4];
    g2r_16<A_KC>(ra, A, p.lda, m0, p.M, 0, p.K);
    g2r_16<B_KC>(rb, B, p.ldb, n0, p.N, 0, p.K);
    r2s_16<A_KC>(ra, As0);
    r2s_16<B_KC>(rb, Bs0);
    __syncthreads();

    const int frow = lane & 15, fk = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            g2r_16<A_KC>(ra, A, p.lda, m0, p.M, (kt + 1) * BK16, p.K);
            g2r_16<B_KC>(rb, B, p.ldb, n0, p.N, (kt + 1) * BK16, p.K);
        }
        const char* Ac = As0 + cur * OPER16_BYTES;
        const char* Bc = Bs0 + cur * OPER16_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm * 64 + i * 16 + frow;
                af[i] = *reinterpret_cast<const bf16x8*>(Ac + swz16(row, s * 4 + fk));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wn * 64 + j * 16 + frow;
                bfr[j] = *reinterpret_cast<const bf16x8*>(Bc + swz16(row, s * 4 + fk));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) {
            r2s_16<A_KC>(ra, As0 + (cur ^ 1) * OPER16_BYTES);
            r2s_16<B_KC>(rb, Bs0 + (cur ^ 1) * OPER16_BYTES);
        }
        __syncthreads();
    }

    // accumulators -> LDS (C/D map of 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg)
    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                const int col = wn * 64 + j * 16 + (lane & 15);
                Cs[row * CS_PITCH + col] = acc[i][j][r];
            }
    float2* rowstat = reinterpret_cast<float2*>(smem + CS_BYTES);          // present when launched with ln_lds(p) extra bytes
    ln_rowstat_fill(p, rowstat, m0, n0, BM, tid, 256);
    __syncthreads();
    if constexpr (A_KC && B_KC) epilogue_any<bf16_t>(p, Cs, m0, n0, LnArgs{rowstat, 0});       // (the other layouts do without the eavqa_gemm_ln form: compile time)
    else epilogue<bf16_t, EpiGeo128, false>(p, Cs, m0, n0);
}


// ===================================================== bf16 fast path ===
// Both operands k-contiguous and K % 32 == 0 (every GEMM of the frozen ViT / LM, forward and dgrad,
// after weight pre-packing).  Differences from the general kernel above:
//   * global -> LDS by LDS-DMA (global_load_lds_dwordx4): no staging registers, no ds_write;
//   * BK = 32, a ring of 4 LDS stages (16 KiB each: A 8 KiB + B 8 KiB), tiles t+1..t+3 in flight
//     while tile t is multiplied; ONE raw s_barrier per K-tile with a counted vmcnt (never 0 in
//     the steady state), so the DMA stays in flight across barriers;
//   * 64-byte LDS rows with the 16-byte chunk XOR-swizzled by (-(row >> 2)) & 3: the 16 lanes of
//     every ds_read_b128 lane group land on 16 different 16-byte slots of the 256-byte bank row.
//     LDS-DMA writes linearly (wave base + lane * 16), so the swizzle is applied to the per-lane
//     SOURCE address and again on the fragment read (same involution);
//   * rows beyond M / N are clamped to the last valid row (their products only reach output rows
//     that are never stored), so no lane is predicated off and the DMA count per wave is exact;
//   * the LDS footprint (ring 64 KiB, C staging 66 KiB) lets two workgroups share a CU;
//   * block -> tile map: each XCD (blockIdx % 8) owns a rectangle of the tile grid so that the
//     A / B panels it re-reads stay in its own 4 MiB L2.
constexpr int FBK = 32;
constexpr int FOPER = 128 * FBK * 2;        // 8 KiB per operand per stage
constexpr int FSTAGE = 2 * FOPER;           // 16 KiB

__device__ __forceinline__ int fswz(int row, int kc) { return row * 64 + ((kc ^ ((-(row >> 2)) & 3)) << 4); }

struct FastMap { int gx, gy; };

__device__ __forceinline__ bool fast_tile(const GemmParams& p, int gx, int gy, int& tm, int& tn) {
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int xi = xcd % gx, yi = xcd / gx;
    const int qm = p.tiles_m / gx, rm = p.tiles_m % gx, qn = p.tiles_n / gy, rn = p.tiles_n % gy;
    const int m_begin = xi * qm + min(xi, rm), m_cnt = qm + (xi < rm ? 1 : 0);
    const int n_begin = yi * qn + min(yi, rn), n_cnt = qn + (yi < rn ? 1 : 0);
    if (m_cnt == 0 || local >= m_cnt * n_cnt) return false;
    tm = m_begin + local % m_cnt;
    tn = n_begin + local / m_cnt;
    return true;
}

// one pipeline step: tile t is already in registers (fragment set P); tile t+1 is fetched from its LDS stage
// into set P^1 while the 16 MFMAs of tile t run, and the DMA of tile t+4 is issued into the stage tile t
// occupied (its fragments left LDS during the previous step).
#define EAVQA_FAST_STEP(P, t)                                                                         \
    {                                                                                                 \
        const int rem = nk - 2 - (t);             /* tiles issued after t+1 */                         \
        /* fragment set P (read during the previous step) is complete; unconditional so that the      */ \
        /* compiler's own lgkmcnt bookkeeping sees it on every path and adds no drain before the MFMAs */ \
        /* sched_barrier: MFMAs are register-only, so the scheduler would otherwise sink the previous  */ \
        /* step's MFMAs below this wait (draining the reads that were just issued)                    */ \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        __builtin_amdgcn_s_waitcnt(0xC07F);       /* lgkmcnt(0) */                                     \
        if ((t) + 1 < nk) {                                                                           \
            /* s_waitcnt simm16 (gfx9): vmcnt [3:0]+[15:14], expcnt [6:4], lgkmcnt [11:8]; the builtin   */ \
            /* (unlike inline asm) is seen by the compiler's own wait-count bookkeeping.  Tiles t+2 ..   */ \
            /* t+NST-1 (4 DMA each) may stay in flight; near the end fewer were issued.                 */ \
            if (ABL < 3) {                                                                            \
            if (rem >= NST - 2) __builtin_amdgcn_s_waitcnt(vm_only(4 * (NST - 2)));                   \
            else if (rem >= 6) __builtin_amdgcn_s_waitcnt(vm_only(24));                               \
            else if (rem == 5) __builtin_amdgcn_s_waitcnt(vm_only(20));                               \
            else if (rem == 4) __builtin_amdgcn_s_waitcnt(vm_only(16));                               \
            else if (rem == 3) __builtin_amdgcn_s_waitcnt(vm_only(12));                               \
            else if (rem == 2) __builtin_amdgcn_s_waitcnt(vm_only(8));                                \
            else if (rem == 1) __builtin_amdgcn_s_waitcnt(vm_only(4));                                \
            else __builtin_amdgcn_s_waitcnt(vm_only(0));                                              \
            __builtin_amdgcn_s_barrier();                                                             \
            }                                                                                         \
            if ((ABL < 1 || ABL >= 4) && (t) + NST < nk) issue((t) + NST);                            \
            if (ABL < 2) {                                                                            \
            const char* st = smem + (((t) + 1) & (NST - 1)) * FSTAGE;                                 \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                             \
                fa[(P) ^ 1][i] = *reinterpret_cast<const bf16x8*>(st + a_off + i * 1024);             \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                             \
                fb[(P) ^ 1][j] = *reinterpret_cast<const bf16x8*>(st + b_off + j * 1024);             \
            } else {                                                                                  \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) { fa[(P) ^ 1][i] = fa[P][i]; fb[(P) ^ 1][i] = fb[P][i]; } \
            }                                                                                         \
        }                                                                                             \
        if (ABL != 4) {                                                                               \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                 \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                             \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[P][i], fb[P][j], acc[i][j], 0, 0, 0); \
        }                                                                                             \
    }

// s_waitcnt immediate for "vmcnt(n) only" (lgkmcnt and expcnt fields at their no-wait maxima)
__device__ __host__ constexpr int vm_only(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }

// NST: stages of the LDS ring (4: 64 KiB, two workgroups per CU; 8: 128 KiB, used when the grid has at most one
// workgroup per CU anyway - twice the bytes in flight per CU lifts the latency-bound LDS-DMA rate).
// ABL (timing experiments only, results are wrong for ABL != 0): 1 = no DMA in the main loop, 2 = also no
// fragment reads, 3 = also no barrier / waits (bare MFMA loop), 4 = DMA + waits + barriers only (no reads, no MFMA)
template <int ABL, int NST>
__global__ __launch_bounds__(256, 2) void gemm_bf16_fast_kernel(GemmParams p, int gx, int gy, int stagger) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int tm, tn;
    if (!fast_tile(p, gx, gy, tm, tn)) return;
    // two workgroups share a CU and would otherwise run in lockstep (same program, same start): delay every
    // other one so that one block's MFMA phase overlaps the other's DMA-issue / LDS-read phase
    if (stagger > 0 && ((blockIdx.x >> 3) & 1))
        for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(8);
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    // per-lane DMA sources: chunk c = wave*64 + lane + 256*i of the [128 rows][4 chunks] image
    const bf16_t* asrc[2];
    const bf16_t* bsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i;
        const int row = c >> 2, pc = c & 3;
        const int kc = pc ^ ((-(row >> 2)) & 3);
        asrc[i] = A + (int64_t)min(m0 + row, p.M - 1) * p.lda + kc * 8;
        bsrc[i] = B + (int64_t)min(n0 + row, p.N - 1) * p.ldb + kc * 8;
    }
    const int dma_off = wave * 1024;     // wave-uniform LDS offset of this wave's 64 chunks

    auto issue = [&](int kt) {
        char* st = smem + (kt & (NST - 1)) * FSTAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off + i * 4096), 16, 0, 0);
            if (ABL != 5 || i == 0 || lane < 16)     // ABL 5: the DMA pattern of a 128 x 80 tile (quarter-wave last piece)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + FOPER + dma_off + i * 4096), 16, 0, 0);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / FBK;
    const int frow = lane & 15, fk = lane >> 4;
    const int a_off = fswz(wm * 64 + frow, fk);          // + i * 16 rows * 64 B
    const int b_off = FOPER + fswz(wn * 64 + frow, fk);
    bf16x8 fa[2][4], fb[2][4];

    // prologue: tiles 0..NST-1 in flight, tile 0 into fragment set 0
#pragma unroll
    for (int i = 0; i < NST; ++i)
        if (i < nk) issue(i);
    {
        const int later = min(nk, NST) - 1;              // tiles issued after tile 0
        if (later >= 7) __builtin_amdgcn_s_waitcnt(vm_only(28));
        else if (later == 6) __builtin_amdgcn_s_waitcnt(vm_only(24));
        else if (later == 5) __builtin_amdgcn_s_waitcnt(vm_only(20));
        else if (later == 4) __builtin_amdgcn_s_waitcnt(vm_only(16));
        else if (later == 3) __builtin_amdgcn_s_waitcnt(vm_only(12));
        else if (later == 2) __builtin_amdgcn_s_waitcnt(vm_only(8));
        else if (later == 1) __builtin_amdgcn_s_waitcnt(vm_only(4));
        else __builtin_amdgcn_s_waitcnt(vm_only(0));
    }
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[0][i] = *reinterpret_cast<const bf16x8*>(smem + a_off + i * 1024);
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[0][j] = *reinterpret_cast<const bf16x8*>(smem + b_off + j * 1024);

    int t = 0;
    for (; t + 1 < nk; t += 2) {
        EAVQA_FAST_STEP(0, t)
        EAVQA_FAST_STEP(1, t + 1)
    }
    if (t < nk) EAVQA_FAST_STEP(0, t)
    __syncthreads();   // every wave is done with the ring before it becomes the C staging tile

    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                const int col = wn * 64 + j * 16 + (lane & 15);
                Cs[row * CS_PITCH + col] = acc[i][j][r];
            }
    __syncthreads();
    epilogue<bf16_t, EpiGeo128, false>(p, Cs, m0, n0);
}
#undef EAVQA_FAST_STEP


typedef void (*fast_kernel_t)(GemmParams, int, int, int);

int launch_fast(const GemmParams& p, hipStream_t stream, const Knobs& kn) {
    // (round 3: the timing-only ablation builds ABL 1..5 of this round-1 kernel are no longer instantiated; the knob field is ignored here)
    static const fast_kernel_t kernels[2] = {gemm_bf16_fast_kernel<0, 4>, gemm_bf16_fast_kernel<0, 8>};
    static std::atomic<bool> configured{false};        // atomic: concurrent first calls only repeat an idempotent call
    if (!configured.load(std::memory_order_acquire)) {
        for (int i = 0; i < 2; ++i)
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[i]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    8 * FSTAGE) != hipSuccess)
                return EAVQA_E_LAUNCH;
        configured.store(true, std::memory_order_release);
    }
    // deep ring (8 stages, one workgroup per CU): measured on MI355X to give no gain over 4 stages even for grids of one
    // tile per CU (the LDS-DMA rate of a CU is a throughput cap, not a bytes-in-flight limit) - kept as an experiment knob
    const bool deep = kn.deep == 2;
    const fast_kernel_t kernel = deep ? kernels[1] : kernels[0];
    const int lds_bytes = deep ? 8 * FSTAGE : CS_BYTES;
    // XCD grid gx x gy = 8 minimising the panels one XCD touches (rows + cols of its rectangle)
    int best_gx = 8, best_cost = 1 << 30;
    const int cand[4] = {8, 4, 2, 1};
    for (int c = 0; c < 4; ++c) {
        const int gx = cand[c], gy = 8 / gx;
        const int cost = (p.tiles_m + gx - 1) / gx + (p.tiles_n + gy - 1) / gy;
        if (cost < best_cost) { best_cost = cost; best_gx = gx; }
    }
    const int gx = best_gx, gy = 8 / gx;
    const int per_xcd = ((p.tiles_m + gx - 1) / gx) * ((p.tiles_n + gy - 1) / gy);
    hipLaunchKernelGGL(kernel, dim3(per_xcd * 8), dim3(256), lds_bytes, stream, p, gx, gy, kn.stagger);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}


// ============================================== bf16 shaped tiles ===
// (16 MF WM) x (16 NF WN) output tile per workgroup of WM x WN waves, same LDS-DMA ring (BK = 32, 4 stages, counted vmcnt,
// one s_barrier per K-step) and register-prefetched fragments as the fast kernel.  Why other shapes: a CU takes in its
// operand tiles at a fixed rate (measured ~52 GB/s into LDS whether one or two workgroups share the CU: K = 5120 takes
// 50 / 51 / 54 us on 80 / 160 / 256 tiles of 128 x 128 and 103 us on 512), so the time of a GEMM is
//     rounds of 256 workgroups  x  (BM + BN) bytes per workgroup and K-step
// and the best tile is the one whose grid just fills the 256 CUs once:
//   * narrow 128 x 80 / 128 x 96 (4 x 1 waves, 2 x NF fragments): N = 1280 at M ~ 2000 is 160 tiles of 128 x 128 (96 CUs
//     idle) but 256 tiles of 128 x 80, each moving 208 / 256 of the bytes;
//   * tall 256 x 128 / 256 x 160 / 256 x 192 (4 x 2 waves, 4 x NF fragments): N = 3840 at M ~ 2000 is 480 tiles of
//     128 x 128 (two rounds) but 240 of 256 x 128 (one round at 384 / 512 of the bytes).
// The B stage (16 NF WN rows x 64 B) is moved by BFULL full-wave DMAs per wave plus, when 4 BN is not a multiple of the
// workgroup size, one piece of BREM lanes per wave, so that every wave issues the same number of DMAs per stage and the
// counted vmcnt waits stay exact.  The C tile leaves through LDS in passes of as many wave rows as fit the ring's bytes.
// block -> tile.  gx > 0: XCD (blockIdx % 8) owns the rectangle (xi, yi) of a gx x gy split of the tile grid (the panels it
// re-reads stay in its L2); gx == 0: XCD owns a contiguous run of ceil / floor(tiles / 8) tiles in M-fastest order (used
// when a rectangle split would put more than 32 tiles on one XCD although the grid fits the chip once).
__device__ __forceinline__ bool shaped_tile(int gx, int gy, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    if (gx == 0) {
        const int nwg = tiles_m * tiles_n, q = nwg >> 3, r = nwg & 7;
        if (local >= q + (xcd < r ? 1 : 0)) return false;
        const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
        tm = wgid % tiles_m;
        tn = wgid / tiles_m;
        return true;
    }
    const int xi = xcd % gx, yi = xcd / gx;
    const int qm = tiles_m / gx, rm = tiles_m % gx, qn = tiles_n / gy, rn = tiles_n % gy;
    const int m_begin = xi * qm + min(xi, rm), m_cnt = qm + (xi < rm ? 1 : 0);
    const int n_begin = yi * qn + min(yi, rn), n_cnt = qn + (yi < rn ? 1 : 0);
    if (m_cnt == 0 || local >= m_cnt * n_cnt) return false;
    tm = m_begin + local % m_cnt;
    tn = n_begin + local / m_cnt;
    return true;
}

// host side of shaped_tile: the split and the number of workgroups the fullest XCD receives
struct GridPlan { int gx, gy, per_xcd; };
inline GridPlan plan_grid(int tiles_m, int tiles_n, int bm, int bn) {
    GridPlan g{8, 1, 0};
    int best_cost = 1 << 30;
    const int cand[4] = {8, 4, 2, 1};
    for (int c = 0; c < 4; ++c) {
        const int gx = cand[c], gy = 8 / gx;
        const int cost = ((tiles_m + gx - 1) / gx) * bm + ((tiles_n + gy - 1) / gy) * bn;     // operand rows one XCD touches
        if (cost < best_cost) { best_cost = cost; g.gx = gx; g.gy = gy; }
    }
    g.per_xcd = ((tiles_m + g.gx - 1) / g.gx) * ((tiles_n + g.gy - 1) / g.gy);
    const int even = (tiles_m * tiles_n + 7) / 8;
    if ((g.per_xcd + 31) / 32 > (even + 31) / 32) { g.gx = 0; g.gy = 0; g.per_xcd = even; }
    return g;
}

template <int WM, int WN, int MF, int NF> struct TileGeo {
    static constexpr int NT = 64 * WM * WN, NW = WM * WN;
    static constexpr int TBM = 16 * MF * WM, TBN = 16 * NF * WN;
    static constexpr int AFULL = 4 * TBM / NT, BFULL = 4 * TBN / NT;
    static constexpr int BREM = (4 * TBN - BFULL * NT) / NW;             // lanes of the partial B piece per wave
    static constexpr int NDMA = AFULL + BFULL + (BREM > 0 ? 1 : 0);      // DMA instructions per wave and stage
    static constexpr int AOPER = TBM * 64, STAGE = (TBM + TBN) * 64, RING = 4 * STAGE;
    static constexpr int PITCH = TBN + 4;
    // wave rows staged per epilogue pass: the most that fit the ring
    static constexpr int SP = (16 * MF * WM * PITCH * 4 <= RING) ? WM : ((16 * MF * (WM / 2) * PITCH * 4 <= RING) ? WM / 2 : 1);
    static constexpr int PROWS = 16 * MF * SP;
    static constexpr int TPR = TBN / 4, RPP = NT / TPR, NPASS = (PROWS + RPP - 1) / RPP;
    static_assert(4 * TBM == AFULL * NT, "A stage must split evenly");
    static_assert(BFULL * NT + BREM * NW == 4 * TBN && BREM < 64, "B stage: full pieces + one partial piece per wave");
    static_assert(16 * MF * PITCH * 4 <= RING, "one wave row of C must fit the ring");
    static_assert(WM % SP == 0, "passes cover whole wave rows");
};

#define EAVQA_SHAPED_STEP(P, t)                                                                       \
    {                                                                                                 \
        const int rem = nk - 2 - (t);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        __builtin_amdgcn_s_waitcnt(0xC07F);       /* lgkmcnt(0): fragment set P is complete */         \
        if ((t) + 1 < nk) {                                                                           \
            if (rem >= 2) __builtin_amdgcn_s_waitcnt(vm_only(2 * G::NDMA));                           \
            else if (rem == 1) __builtin_amdgcn_s_waitcnt(vm_only(G::NDMA));                          \
            else __builtin_amdgcn_s_waitcnt(vm_only(0));                                              \
            __builtin_amdgcn_s_barrier();                                                             \
            if ((t) + 4 < nk) issue((t) + 4);                                                         \
            const char* st = smem + (((t) + 1) & 3) * G::STAGE;                                       \
            _Pragma("unroll") for (int i = 0; i < MF; ++i)                                            \
                fa[(P) ^ 1][i] = *reinterpret_cast<const bf16x8*>(st + a_off + i * 1024);             \
            _Pragma("unroll") for (int j = 0; j < NF; ++j)                                            \
                fb[(P) ^ 1][j] = *reinterpret_cast<const bf16x8*>(st + b_off + j * 1024);             \
        }                                                                                             \
        _Pragma("unroll") for (int i = 0; i < MF; ++i)                                                \
            _Pragma("unroll") for (int j = 0; j < NF; ++j)                                            \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[P][i], fb[P][j], acc[i][j], 0, 0, 0); \
    }

template <int WM, int WN, int MF, int NF>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN <= 4) ? 2 : 1) void gemm_bf16_shaped_kernel(GemmParams p, int gx, int gy, int tiles_m, int tiles_n) {
    using G = TileGeo<WM, WN, MF, NF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int tm, tn;
    if (!shaped_tile(gx, gy, tiles_m, tiles_n, tm, tn)) return;
    const int m0 = tm * G::TBM, n0 = tn * G::TBN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    // per-lane DMA sources; chunk c of an operand image is (row c >> 2, physical 16-byte slot c & 3)
    auto src_of = [&](const bf16_t* X, int64_t ld, int row0, int rows_max, int c) {
        const int row = c >> 2, pc = c & 3;
        return X + (int64_t)min(row0 + row, rows_max - 1) * ld + (pc ^ ((-(row >> 2)) & 3)) * 8;
    };
    const bf16_t* asrc[G::AFULL];
    const bf16_t* bsrc[G::BFULL + 1];
#pragma unroll
    for (int i = 0; i < G::AFULL; ++i) asrc[i] = src_of(A, p.lda, m0, p.M, tid + G::NT * i);
#pragma unroll
    for (int i = 0; i < G::BFULL; ++i) bsrc[i] = src_of(B, p.ldb, n0, p.N, tid + G::NT * i);
    bsrc[G::BFULL] = src_of(B, p.ldb, n0, p.N, G::BFULL * G::NT + wave * G::BREM + min(lane, max(G::BREM, 1) - 1));
    const int dma_off = wave * 1024;                                        // + i * NT * 16 for full pieces
    const int dma_off_x = G::AOPER + G::BFULL * G::NT * 16 + wave * G::BREM * 16;

    auto issue = [&](int kt) {
        char* st = smem + (kt & 3) * G::STAGE;
#pragma unroll
        for (int i = 0; i < G::AFULL; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off + i * G::NT * 16), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < G::BFULL; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + G::AOPER + dma_off + i * G::NT * 16), 16, 0, 0);
        if (G::BREM > 0 && lane < G::BREM)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[G::BFULL] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off_x), 16, 0, 0);
    };

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / FBK;
    const int frow = lane & 15, fk = lane >> 4;
    const int a_off = fswz(wm * 16 * MF + frow, fk);                   // + i * 16 rows * 64 B
    const int b_off = G::AOPER + fswz(wn * 16 * NF + frow, fk);        // + j * 16 rows * 64 B
    bf16x8 fa[2][MF], fb[2][NF];

#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < nk) issue(i);
    {
        const int later = min(nk, 4) - 1;
        if (later == 3) __builtin_amdgcn_s_waitcnt(vm_only(3 * G::NDMA));
        else if (later == 2) __builtin_amdgcn_s_waitcnt(vm_only(2 * G::NDMA));
        else if (later == 1) __builtin_amdgcn_s_waitcnt(vm_only(G::NDMA));
        else __builtin_amdgcn_s_waitcnt(vm_only(0));
    }
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < MF; ++i) fa[0][i] = *reinterpret_cast<const bf16x8*>(smem + a_off + i * 1024);
#pragma unroll
    for (int j = 0; j < NF; ++j) fb[0][j] = *reinterpret_cast<const bf16x8*>(smem + b_off + j * 1024);

    int t = 0;
    for (; t + 1 < nk; t += 2) {
        EAVQA_SHAPED_STEP(0, t)
        EAVQA_SHAPED_STEP(1, t + 1)
    }
    if (t < nk) EAVQA_SHAPED_STEP(0, t)
    __syncthreads();

    float* Cs = reinterpret_cast<float*>(smem);
    for (int pass = 0; pass < WM / G::SP; ++pass) {
        if (wm / G::SP == pass) {
            const int r0 = (wm % G::SP) * 16 * MF;
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + i * 16 + (lane >> 4) * 4 + r;
                        const int col = wn * 16 * NF + j * 16 + (lane & 15);
                        Cs[row * G::PITCH + col] = acc[i][j][r];
                    }
        }
        __syncthreads();
        epilogue<bf16_t, EpiGeo<G::TPR, G::RPP, G::NPASS, G::PITCH, G::PROWS>, false>(p, Cs, m0 + pass * G::PROWS, n0);
        if (pass + 1 < WM / G::SP) __syncthreads();
    }
}
#undef EAVQA_SHAPED_STEP

template <int WM, int WN, int MF, int NF>
int launch_shaped(const GemmParams& p, hipStream_t stream) {
    using G = TileGeo<WM, WN, MF, NF>;
    static std::atomic<bool> configured{false};        // atomic: concurrent first calls only repeat an idempotent call
    if (!configured.load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_shaped_kernel<WM, WN, MF, NF>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, G::RING) != hipSuccess)
            return EAVQA_E_LAUNCH;
        configured.store(true, std::memory_order_release);
    }
    const int tiles_m = (p.M + G::TBM - 1) / G::TBM, tiles_n = (p.N + G::TBN - 1) / G::TBN;
    const GridPlan g = plan_grid(tiles_m, tiles_n, G::TBM, G::TBN);
    hipLaunchKernelGGL((gemm_bf16_shaped_kernel<WM, WN, MF, NF>), dim3(g.per_xcd * 8), dim3(G::NT), G::RING, stream, p, g.gx, g.gy,
                       tiles_m, tiles_n);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}


// `rate`: measured ns per 64-byte operand row and K-step (32) of one workgroup alone on a CU (K = 5120 probes and the
// cfg2 shapes, tools/gemm_bench.py): the wider 8-wave tiles get closer to the MFMA / LDS limits and pay more per byte.
struct ShapeChoice { int bm, bn; float rate; int (*launch)(const GemmParams&, hipStream_t); };
const ShapeChoice SHAPES[5] = {
    {128, 80, 1.17f, launch_shaped<4, 1, 2, 5>}, {128, 96, 1.20f, launch_shaped<4, 1, 2, 6>},
    {256, 128, 1.15f, launch_shaped<4, 2, 4, 4>}, {256, 160, 1.23f, launch_shaped<4, 2, 4, 5>}, {256, 192, 1.39f, launch_shaped<4, 2, 4, 6>},
};
constexpr float RATE_FAST = 1.245f, RATE_BIG = 1.27f;

// Modelled time (ns, without the launch) of a grid of bm x bn tiles: the fullest XCD's workgroups per CU (co-resident
// ones share the CU's intake rate) x (operand bytes per K-step at that rate + the tile's epilogue).  Calibrated on MI355X
// (128 x 128: 17.8 us at K = 1280, 51.9 us at K = 5120; 256 x 128 on 240 tiles: 29 us at K = 1280).
inline float tile_cost(const GemmParams& p, int bm, int bn, float rate) {
    const int tiles_m = (p.M + bm - 1) / bm, tiles_n = (p.N + bn - 1) / bn;
    const GridPlan g = plan_grid(tiles_m, tiles_n, bm, bn);
    const float rounds = float((g.per_xcd + 31) / 32);
    return rounds * (rate * (bm + bn) * (p.K / 32) + 0.25f * bm * bn);
}

// ====================================================== bf16 big tiles ===
// 256 x 256 output tile per 1024-thread workgroup (16 waves as 4 x 4, 64 x 64 each, four waves per SIMD) for GEMMs
// with enough columns to give most CUs a tile (N >= 3840 on the hot path: QKV, FFN up, lm_head; the CLIP tower and
// the few-shot prefill).  Why: with 128 x 128 tiles every FLOP costs 1/64 B of L2 -> LDS traffic and the LDS-DMA path
// of a CU saturates near 30 B/clk, well before the matrix pipe; a 256 x 256 tile halves that (1/128 B per FLOP) and
// four waves per SIMD hide the fragment-read latency without a second register set.
//   * BK = 64: LDS rows are full 128-byte lines (every DMA instruction moves 8 whole rows), XOR swizzle chunk ^= row & 7;
//   * 2 stages x 64 KiB; tile t+1 is fetched (LDS-DMA) while tile t multiplies (32 MFMAs per wave ~ 2048 cycles per
//     SIMD, which covers an L2 round trip); one s_barrier per K-tile;
//   * the C tile leaves through LDS one 64-row slab at a time (the accumulators of one wave row).
constexpr int GBM = 256, GBN = 256, GBK = 64;
constexpr int BIG_GROUP_N = 8;                     // tile columns per group of the in-XCD order (tools/gemm_bench.py --group-n sweep, profiles/round3_tile_order.md)
constexpr int GOPER = GBM * GBK * 2;               // 32 KiB per operand per stage
constexpr int GSTAGE = 2 * GOPER;                  // 64 KiB
constexpr int GCS_PITCH = GBN + 4;                 // floats per staged C row
constexpr int GLDS_BYTES = 2 * GSTAGE;             // 128 KiB (the 64 x 260 fp32 slab reuses it)
using EpiGeo256 = EpiGeo<64, 16, 4, GCS_PITCH, 64, 1>;    // 64 x 256 slab, 1024 threads (128 registers per lane: one pass at a time in the eavqa_gemm_ln form)

// Order of an XCD's tiles in time (its 32 CUs take them in `local` order): column groups of GN tile columns, inside a group n
// fastest.  The 32 tiles in flight are then 32 / GN tile rows x GN columns: every A panel is shared by GN concurrent tiles and the
// group's GN B panels stay in the XCD's L2 while the rows stream by - with m fastest (round 2) a multi-round problem re-read
// every A panel once per tile column from beyond L2 (FFN-down of the CLIP tower: 4 columns -> the 337 MB A operand four times).
__device__ __forceinline__ bool big_tile(const GemmParams& p, int gx, int gy, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int xi = xcd % gx, yi = xcd / gx;
    const int qm = tiles_m / gx, rm = tiles_m % gx, qn = tiles_n / gy, rn = tiles_n % gy;
    const int m_begin = xi * qm + min(xi, rm), m_cnt = qm + (xi < rm ? 1 : 0);
    const int n_begin = yi * qn + min(yi, rn), n_cnt = qn + (yi < rn ? 1 : 0);
    if (m_cnt == 0 || local >= m_cnt * n_cnt) return false;
    const int GN = p.group_n;
    if (GN <= 0) {                                     // m fastest (round 2 order; one-round problems do not care)
        tm = m_begin + local % m_cnt;
        tn = n_begin + local / m_cnt;
        return true;
    }
    const int per_group = m_cnt * GN;
    const int g = local / per_group, r = local - g * per_group;
    const int gn = min(GN, n_cnt - g * GN);           // columns of this (possibly last, narrower) group
    tm = m_begin + r / gn;
    tn = n_begin + g * GN + r % gn;
    return true;
}

template <bool LNX>
__global__ __launch_bounds__(1024) void gemm_bf16_big_kernel(typename KernArg<LNX>::type pk, int gx, int gy, int tiles_m, int tiles_n) {
    const GemmParams p = widen(pk);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int tm, tn;
    if (!big_tile(p, gx, gy, tiles_m, tiles_n, tm, tn)) return;
    const int m0 = tm * GBM, n0 = tn * GBN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    // DMA sources: chunk c = tid + 1024 i of the [256 rows][8 chunks] image (row = c >> 3, physical chunk c & 7)
    const bf16_t* asrc[2];
    const bf16_t* bsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 1024 * i;
        const int row = c >> 3, pc = c & 7;
        asrc[i] = A + (int64_t)min(m0 + row, p.M - 1) * p.lda + (pc ^ (row & 7)) * 8;
        bsrc[i] = B + (int64_t)min(n0 + row, p.N - 1) * p.ldb + (pc ^ (row & 7)) * 8;
    }
    const int dma_off = wave * 1024;
    auto issue = [&](int kt) {
        char* st = smem + (kt & 1) * GSTAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + kt * GBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off + i * 16384), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + kt * GBK),
                                             (__attribute__((address_space(3))) void*)(st + GOPER + dma_off + i * 16384), 16, 0, 0);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / GBK;
    const int frow = lane & 15, fk = lane >> 4;
    const int arow = wm * 64 + frow, brow = wn * 64 + frow;     // + 16 i ; row & 7 == frow & 7 for every fragment
    issue(0);
    float2* rowstat = reinterpret_cast<float2*>(smem + GLDS_BYTES);     // eavqa_gemm_ln: under the first tile's round trip
    if (LNX) ln_rowstat_fill(p, rowstat, m0, n0, GBM, tid, 1024);
    for (int kt = 0; kt < nk; ++kt) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0070);        // vmcnt(0) lgkmcnt(0): this wave's share of tile kt has landed
        __builtin_amdgcn_s_barrier();              // ... and everybody's; all reads of the other stage are done
        if (kt + 1 < nk) issue(kt + 1);
        const char* st = smem + (kt & 1) * GSTAGE;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 af[4], bfr[4];
            const int sw = ((s * 4 + fk) ^ (frow & 7)) << 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8*>(st + (arow + 16 * i) * 128 + sw);
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(st + GOPER + (brow + 16 * j) * 128 + sw);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();

    float* Cs = reinterpret_cast<float*>(smem);
    for (int slab = 0; slab < 4; ++slab) {
        if (wm == slab) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = i * 16 + (lane >> 4) * 4 + r;
                        const int col = wn * 64 + j * 16 + (lane & 15);
                        Cs[row * GCS_PITCH + col] = acc[i][j][r];
                    }
        }
        __syncthreads();
        epilogue<bf16_t, EpiGeo256, LNX>(p, Cs, m0 + slab * 64, n0, LnArgs{rowstat, slab * 64});
        __syncthreads();
    }
}

// XCD rectangle of the 256 x 256 kernel: gx x gy XCDs over tile rows x tile columns with the fewest panels per XCD; returns tiles per XCD
// (round 3: fewest ROUNDS of 32 workgroups per XCD first - the few-shot prefill's FFN-up, 19 x 40 tiles, is 10 x 10 = 100 tiles per XCD =
// four rounds on the 2 x 4 rectangle with the fewest panels but 19 x 5 = 95 = three rounds on 1 x 8 - then the fewest panels)
inline int big_grid(int tiles_m, int tiles_n, int& gx, int& gy) {
    int best_gx = 8, best_cost = 1 << 30, best_rounds = 1 << 30;
    const int cand[4] = {8, 4, 2, 1};
    for (int c = 0; c < 4; ++c) {
        const int x = cand[c], y = 8 / x;
        const int pm = (tiles_m + x - 1) / x, pn = (tiles_n + y - 1) / y;
        const int rounds = (pm * pn + 31) / 32, cost = pm + pn;
        if (rounds < best_rounds || (rounds == best_rounds && cost < best_cost)) { best_rounds = rounds; best_cost = cost; best_gx = x; }
    }
    gx = best_gx; gy = 8 / gx;
    return ((tiles_m + gx - 1) / gx) * ((tiles_n + gy - 1) / gy);
}

int launch_big(const GemmParams& p, hipStream_t stream) {
    static std::atomic<bool> configured{false};        // atomic: concurrent first calls only repeat an idempotent call
    if (!configured.load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_big_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                GLDS_BYTES) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_big_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                GLDS_BYTES + LN_ROWSTAT_BYTES) != hipSuccess)
            return EAVQA_E_LAUNCH;
        configured.store(true, std::memory_order_release);
    }
    const int tiles_m = (p.M + GBM - 1) / GBM, tiles_n = (p.N + GBN - 1) / GBN;
    int gx, gy;
    const int per_xcd = big_grid(tiles_m, tiles_n, gx, gy);
    if (p.ln_stats || p.stats_out || p.copy_out)        // eavqa_gemm_ln: its own instantiation (the plain one has no registers to spare)
        hipLaunchKernelGGL(gemm_bf16_big_kernel<true>, dim3(per_xcd * 8), dim3(1024), GLDS_BYTES + ln_lds(p), stream, p, gx, gy, tiles_m, tiles_n);
    else
        hipLaunchKernelGGL(gemm_bf16_big_kernel<false>, dim3(per_xcd * 8), dim3(1024), GLDS_BYTES, stream, p, gx, gy, tiles_m, tiles_n);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

// Rows to hand to a second, small-tile launch (0 = none): when the last tile row is ragged (M % 256 <= 192 rows) and the problem without it
// needs one round of workgroups less.  The CLIP tower at 64 images is M = 16 448 = 64 tile rows + 64 rows: out-proj / FFN-down are 260
// tiles = TWO rounds for 256 CUs (the second one of four tiles), QKV 780 = four rounds instead of three; at 160 images FFN-up is 2 576
// tiles = eleven rounds instead of ten.  Every tile costs the same whatever its valid rows, so the few ragged rows cost a whole round.
inline int big_split_rows(int M, int N) {
    const int rem = M % GBM;
    if (rem == 0 || rem > 192 || M <= GBM) return 0;
    int gx, gy;
    const int tiles_n = (N + GBN - 1) / GBN;
    const int with = (big_grid((M + GBM - 1) / GBM, tiles_n, gx, gy) + 31) / 32, without = (big_grid(M / GBM, tiles_n, gx, gy) + 31) / 32;
    return without < with ? rem : 0;
}

bool use_big(const GemmParams& p, const Knobs& kn) {
    if (p.K % GBK) return false;
    if (kn.big_mode == 1) return false;
    if (kn.big_mode == 2) return true;
    const int tiles = ((p.M + GBM - 1) / GBM) * ((p.N + GBN - 1) / GBN);
    return tiles >= 144;     // measured crossover on MI355X: below ~140 tiles the 128 x 128 kernel (more CUs busy) wins
}


// ============================================== bf16 full-line tiles ===
#include "gemm_k64.hip"

// Dispatcher's model of a specialised tile on this problem (ns): a fixed part (launch ramp, first tile's round trip, C staging
// and stores) + K-steps x rows per step x the tile's rate, times the workgroups the fullest CU receives.  Calibrated on MI355X
// (profiles/round2_gemm_k64.md): 4-consumer tiles take in a 128-byte operand row per 1.56 ns, 8-consumer tiles per 1.95 ns (they
// are close to their MFMA time), 128 x 128 per 1.73 ns; fixed ~4.5 us + 0.1 ns per output element of the tile.
inline float k64_cost(const GemmParams& p, const K64Choice& c, float* multi_round_loop = nullptr) {
    const int tiles_m = (p.M + c.bm - 1) / c.bm, tiles_n = (p.N + c.bn - 1) / c.bn;
    const GridPlan g = plan_grid(tiles_m, tiles_n, c.bm, c.bn);
    const float rounds = float((g.per_xcd + 31) / 32);
    const float loop = rounds * c.rate * (c.bm + c.bn) * (p.K / 64);
    if (multi_round_loop) *multi_round_loop = rounds > 1.f ? loop : 0.f;
    return loop + rounds * 0.1f * c.bm * c.bn + 4500.f;
}

#include "gemm_fp8.hip"

// ======================================================= bf16 skinny M ===
// M <= 64 rows (a decode step: M = batch; the MLP mapper at batch 64): the GEMM is a weight-streaming problem, HBM
// bound on B.  Each workgroup owns 16 output columns and its 8 waves split K; a wave loads its B fragment (16 rows x
// 32 k, 16 B per lane) and the matching A fragments straight into VGPRs (no LDS round trip: nothing is shared between
// waves), eight K-steps unrolled so that >= 16 loads are in flight per wave, one MFMA per A fragment and step.
// The 8 partial tiles are summed through LDS and a scalar epilogue (same semantics as the tiled kernels) writes the
// 16 x M results.  Algorithmic bytes: N*K*2 (weights) once; A (<= 64 x K) is re-read from L2 by every workgroup.
template <int MF>
__global__ __launch_bounds__(512) void gemm_bf16_skinny_kernel(GemmParams p) {
    __shared__ float red[8][64][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);
    const int nsteps = p.K >> 5;
    const int per_wave = (nsteps + 7) >> 3;
    const int s_begin = wave * per_wave, s_end = min(nsteps, s_begin + per_wave);
    const bf16_t* bp = B + (int64_t)min(n0 + x, p.N - 1) * p.ldb + 8 * g;
    const bf16_t* ap[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) ap[f] = A + (int64_t)min(16 * f + x, p.M - 1) * p.lda + 8 * g;
    f32x4 acc[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int s = s_begin;
    for (; s + 8 <= s_end; s += 8) {
        bf16x8 b[8], a[8][MF];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            b[u] = *reinterpret_cast<const bf16x8*>(bp + (s + u) * 32);
#pragma unroll
            for (int f = 0; f < MF; ++f) a[u][f] = *reinterpret_cast<const bf16x8*>(ap[f] + (s + u) * 32);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int f = 0; f < MF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][f], b[u], acc[f], 0, 0, 0);
    }
    for (; s < s_end; ++s) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(bp + s * 32);
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap[f] + s * 32);
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[f], 0, 0, 0);
        }
    }
    // C fragment: row m = 16 f + 4 g + r, column n = n0 + x
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][16 * f + 4 * g + r][x] = acc[f][r];
    __syncthreads();
    for (int e = tid; e < MF * 16 * 16; e += 512) {
        const int m = e >> 4, c = e & 15, n = n0 + c;
        if (m >= p.M || n >= p.N) continue;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += red[w][m][c];
        v = p.alpha * v + (p.bias ? p.bias[n] : 0.f);
        const int64_t ia = (int64_t)m * p.ld_aux + n;
        if (p.aux_out) elem<bf16_t>::st(reinterpret_cast<bf16_t*>(p.aux_out) + ia, v);
        if (p.aux_in) v *= act_bwd(p.act, elem<bf16_t>::ld(reinterpret_cast<const bf16_t*>(p.aux_in) + ia));
        else v = act_fwd(p.act, v);
        if (p.residual) v += p.res_lowp == 2 ? elem<f16_t>::ld(reinterpret_cast<const f16_t*>(p.residual) + (int64_t)m * p.ldr + n)
                             : p.res_lowp ? elem<bf16_t>::ld(reinterpret_cast<const bf16_t*>(p.residual) + (int64_t)m * p.ldr + n)
                                          : reinterpret_cast<const float*>(p.residual)[(int64_t)m * p.ldr + n];
        if (p.out_f32) reinterpret_cast<float*>(p.C)[(int64_t)m * p.ldc + n] = v;
        else if (p.out_f16) elem<f16_t>::st(reinterpret_cast<f16_t*>(p.C) + (int64_t)m * p.ldc + n, v);
        else elem<bf16_t>::st(reinterpret_cast<bf16_t*>(p.C) + (int64_t)m * p.ldc + n, v);
    }
}

int launch_skinny(const GemmParams& p, hipStream_t stream) {
    const int blocks = (p.N + 15) / 16;
    const int mf = (p.M + 15) / 16;
    if (mf == 1) hipLaunchKernelGGL(gemm_bf16_skinny_kernel<1>, dim3(blocks), dim3(512), 0, stream, p);
    else if (mf == 2) hipLaunchKernelGGL(gemm_bf16_skinny_kernel<2>, dim3(blocks), dim3(512), 0, stream, p);
    else if (mf == 3) hipLaunchKernelGGL(gemm_bf16_skinny_kernel<3>, dim3(blocks), dim3(512), 0, stream, p);
    else hipLaunchKernelGGL(gemm_bf16_skinny_kernel<4>, dim3(blocks), dim3(512), 0, stream, p);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

// ================================================================ f32 ===
constexpr int BK32 = 16;
constexpr int PITCH32 = 17;                                  // floats per staged row
constexpr int OPER32_FLOATS = 128 * PITCH32;                 // 2176 floats = 8704 B

template <bool KC>
__device__ __forceinline__ void g2r_32(float4 (&r)[2], const float* X, int64_t ld, int row0, int rows_max,
                                       int k0, int K) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (KC) {
            const int row = c >> 2, kc = c & 3;
            const int gr = row0 + row, gk = k0 + kc * 4;
            if (gr < rows_max && gk < K) v = *reinterpret_cast<const float4*>(X + (int64_t)gr * ld + gk);
        } else {
            const int k = c >> 5, rc = c & 31;
            const int gk = k0 + k, gr = row0 + rc * 4;
            if (gk < K && gr < rows_max) v = *reinterpret_cast<const float4*>(X + (int64_t)gk * ld + gr);
        }
        r[i] = v;
    }
}
template <bool KC>
__device__ __forceinline__ void r2s_32(const float4 (&r)[2], float* S) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i;
        const float w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
        if (KC) {
            const int row = c >> 2, kc = c & 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) S[row * PITCH32 + kc * 4 + j] = w[j];
        } else {
            const int k = c >> 5, rc = c & 31;
#pragma unroll
            for (int j = 0; j < 4; ++j) S[(rc * 4 + j) * PITCH32 + k] = w[j];
        }
    }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sm = reinterpret_cast<float*>(smem);
    float* const As0 = sm;
    float* const Bs0 = sm + 2 * OPER32_FLOATS;

    int tm, tn;
    tile_coords(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const float* A = reinterpret_cast<const float*>(p.A);
    const float* B = reinterpret_cast<const float*>(p.B);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (p.K + BK32 - 1) / BK32;
    float4 ra[2], rb[2];
    g2r_32<A_KC>(ra, A, p.lda, m0, p.M, 0, p.K);
    g2r_32<B_KC>(rb, B, p.ldb, n0, p.N, 0, p.K);
    r2s_32<A_KC>(ra, As0);
    r2s_32<B_KC>(rb, Bs0);
    __syncthreads();

    const int frow = lane & 31, fk = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            g2r_32<A_KC>(ra, A, p.lda, m0, p.M, (kt + 1) * BK32, p.K);
            g2r_32<B_KC>(rb, B, p.ldb, n0, p.N, (kt + 1) * BK32, p.K);
        }
        const float* Ac = As0 + cur * OPER32_FLOATS;
        const float* Bc = Bs0 + cur * OPER32_FLOATS;
#pragma unroll
        for (int s = 0; s < BK32 / 2; ++s) {
            float af[2], bfr[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = Ac[(wm * 64 + i * 32 + frow) * PITCH32 + s * 2 + fk];
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = Bc[(wn * 64 + j * 32 + frow) * PITCH32 + s * 2 + fk];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) {
            r2s_32<A_KC>(ra, As0 + (cur ^ 1) * OPER32_FLOATS);
            r2s_32<B_KC>(rb, Bs0 + (cur ^ 1) * OPER32_FLOATS);
        }
        __syncthreads();
    }

    // C/D map of 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int col = wn * 64 + j * 32 + (lane & 31);
                Cs[row * CS_PITCH + col] = acc[i][j][r];
            }
    float2* rowstat = reinterpret_cast<float2*>(smem + CS_BYTES);          // present when launched with ln_lds(p) extra bytes
    ln_rowstat_fill(p, rowstat, m0, n0, BM, tid, 256);
    __syncthreads();
    if constexpr (A_KC && B_KC) epilogue_any<float>(p, Cs, m0, n0, LnArgs{rowstat, 0});
    else epilogue<float, EpiGeo128, false>(p, Cs, m0, n0);
}

typedef void (*gemm_kernel_t)(GemmParams);

int launch(gemm_kernel_t kernel, const GemmParams& p, hipStream_t stream) {
    // dynamic LDS above 64 KiB must be opted into once per kernel; remember which ones were
    // (idempotent, so a race between host threads only repeats the call)
    static std::atomic<gemm_kernel_t> configured[8];      // zero-initialised; a slot is claimed by compare-exchange
    bool done = false;
    for (int i = 0; i < 8; ++i) done |= (configured[i].load(std::memory_order_acquire) == kernel);
    if (!done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CS_BYTES + LN_ROWSTAT_BYTES) != hipSuccess)
            return EAVQA_E_LAUNCH;
        for (int i = 0; i < 8; ++i) {
            gemm_kernel_t expected = nullptr;
            if (configured[i].compare_exchange_strong(expected, kernel, std::memory_order_acq_rel) || expected == kernel) break;
        }
    }
    const int nwg = p.tiles_m * p.tiles_n;
    hipLaunchKernelGGL(kernel, dim3(nwg), dim3(256), CS_BYTES + ln_lds(p), stream, p);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}


}  // namespace

namespace {
// rows [r0, ...) of an eavqa_gemm_ln argument block (the second launch of a row-split problem)
eavqa_gemm_ln_t ln_rows_from(const eavqa_gemm_ln_t& x, int64_t r0, size_t esz) {
    eavqa_gemm_ln_t y = x;
    if (x.copy_out) y.copy_out = static_cast<char*>(x.copy_out) + (size_t)r0 * (size_t)x.ld_copy * esz;
    if (x.stats_out) y.stats_out = x.stats_out + (size_t)r0 * (size_t)x.stats_ld * 2;
    if (x.ln_stats) y.ln_stats = x.ln_stats + (size_t)r0 * (size_t)x.ln_ld * 2;
    if (x.mean_out) y.mean_out = x.mean_out + r0;
    if (x.rstd_out) y.rstd_out = x.rstd_out + r0;
    return y;
}

int gemm_impl(int dtype, int a_kc, int b_kc, int M, int N, int K,
              const void* A, int64_t lda, const void* B, int64_t ldb,
              void* C, int64_t ldc, int out_flags, float alpha,
              const float* bias, int act,
              const void* aux_in, void* aux_out, int64_t ld_aux,
              const void* residual, int64_t ldr, const eavqa_gemm_ln_t* ln, void* stream, int knobs,
              const void* pf_ptr = nullptr, int64_t pf_bytes = 0) {
    const Knobs kn(knobs);
    const bool ln_consumer = ln && ln->ln_stats;
    if (ln) {
        if (ln->copy_out && ln->ld_copy < N) return EAVQA_E_ARG;
        if (ln->stats_out && ln->stats_ld < (N + 63) / 64) return EAVQA_E_ARG;
        if (ln_consumer && (!ln->ln_c || ln->ln_parts <= 0 || ln->ln_ld < ln->ln_parts || ln->ln_cols <= 0 || !(ln->ln_eps >= 0.f))) return EAVQA_E_ARG;
        if ((ln->mean_out != nullptr) != (ln->rstd_out != nullptr) || (ln->mean_out && !ln_consumer)) return EAVQA_E_ARG;
        if (!(a_kc && b_kc)) return EAVQA_E_SHAPE;          // the eavqa_gemm_ln form exists for k-contiguous operands (the frozen LM's Linear layers)
    }
    if (out_flags & ~(EAVQA_GEMM_OUT_F32 | EAVQA_GEMM_RESIDUAL_LOWP | EAVQA_GEMM_STREAM_F16)) return EAVQA_E_ARG;
    if ((out_flags & (EAVQA_GEMM_RESIDUAL_LOWP | EAVQA_GEMM_STREAM_F16)) && dtype != EAVQA_BF16) return EAVQA_E_DTYPE;   // 16-bit streams: bf16 operands only
    const int out_f32 = out_flags & EAVQA_GEMM_OUT_F32;
    const int stream_f16 = (out_flags & EAVQA_GEMM_STREAM_F16) != 0;
    const int res_lowp = (out_flags & EAVQA_GEMM_RESIDUAL_LOWP) ? (stream_f16 ? 2 : 1) : 0;
    if (!A || !B || !C) return EAVQA_E_ARG;
    if (M <= 0 || N <= 0 || K <= 0) return EAVQA_E_ARG;
    if (dtype != EAVQA_F32 && dtype != EAVQA_BF16) return EAVQA_E_DTYPE;
    if (act < EAVQA_ACT_NONE || act > EAVQA_ACT_QUICK_GELU) return EAVQA_E_DTYPE;
    const int vec = dtype == EAVQA_BF16 ? 8 : 4;
    // the contiguous memory dimension of each operand is read in 16-byte chunks
    const int a_contig = a_kc ? K : M, b_contig = b_kc ? K : N;
    if (a_contig % vec || b_contig % vec) return EAVQA_E_SHAPE;
    if (lda % vec || ldb % vec) return EAVQA_E_ALIGN;
    if (!eavqa_aligned16(A) || !eavqa_aligned16(B)) return EAVQA_E_ALIGN;
    if (lda < a_contig || ldb < b_contig || ldc < N) return EAVQA_E_ARG;
    if ((aux_in || aux_out) && ld_aux < N) return EAVQA_E_ARG;
    if (residual && ldr < N) return EAVQA_E_ARG;

    GemmParams p;
    p.A = A; p.B = B; p.C = C; p.bias = bias; p.aux_in = aux_in; p.aux_out = aux_out; p.residual = residual; p.row_scale = nullptr; p.ablate = kn.ablate;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ld_aux = ld_aux; p.ldr = ldr;
    p.act = act; p.out_f32 = out_f32; p.res_lowp = res_lowp; p.out_f16 = stream_f16 && !out_f32; p.alpha = alpha;
    p.group_n = kn.group_n == 0 ? BIG_GROUP_N : kn.group_n - 1;
    p.tiles_m = (M + BM - 1) / BM;
    p.tiles_n = (N + BN - 1) / BN;
    const int esz = dtype == EAVQA_BF16 ? 2 : 4;
    auto vec_ok = [](const void* ptr, int64_t ld, int bytes_per_elem) {
        return ((reinterpret_cast<uintptr_t>(ptr) % (4 * bytes_per_elem)) == 0) && (ld % 4 == 0);
    };
    p.vec_c = vec_ok(C, ldc, out_f32 ? 4 : esz);
    p.vec_aux = vec_ok(aux_in ? aux_in : aux_out, ld_aux, esz);
    p.vec_res = vec_ok(residual, ldr, res_lowp ? esz : 4);
    p.vec_bias = (reinterpret_cast<uintptr_t>(bias) % 16) == 0;
    if (ln) {
        p.copy_out = ln->copy_out; p.ld_copy = ln->ld_copy; p.vec_copy = ln->copy_out ? vec_ok(ln->copy_out, ln->ld_copy, esz) : 0;
        p.stats_out = ln->stats_out; p.stats_ld = ln->stats_ld;
        if (ln_consumer) {
            p.ln_stats = ln->ln_stats; p.ln_parts = ln->ln_parts; p.ln_ld = ln->ln_ld; p.ln_c = ln->ln_c;
            p.ln_inv_n = 1.0f / float(ln->ln_cols); p.ln_eps = ln->ln_eps; p.mean_out = ln->mean_out; p.rstd_out = ln->rstd_out;
        }
    }
    // the look-ahead region: honoured by the full-line tiles the dispatcher picks from, ignored (correct, only cold) by every other kernel
    if (pf_ptr && pf_bytes > 0 && !ln) { p.pf_ptr = pf_ptr; p.pf_bytes = pf_bytes; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_BF16) {
        if (a_kc && b_kc && (K % 64) == 0 && kn.k64_mode >= 2 && kn.k64_mode < 2 + N_K64) return K64_SHAPES[kn.k64_mode - 2].launch(p, s);
        // M <= 64 with few columns (T5 decoder passes at one or two tokens: N = 2048 is 26 tiles of 128 x 80 for 256 CUs): the 16-column
        // weight-streaming kernel has N / 16 workgroups - 8.7 against 15.1 us at N = K = 2048, 20.9 against 31.9 us at K = 5120 (cold
        // weights); from N = 6144 on the tiles win again (16.6 against 22.3 us at N = 10240)
        const bool few_columns = kn.k64_mode == 0 && kn.shape_mode == 0 && kn.big_mode == 0 && N <= 4096;
        if (!ln && a_kc && b_kc && !kn.disable_fast && M <= 64 && (K % 32) == 0 && N >= 64 && (kn.k64_mode == 1 || (K % 64) != 0 || few_columns)) return launch_skinny(p, s);
        // Default dispatch (K % 64 == 0): the loader / consumer specialised full-line tile the cost model ranks first, or the
        // round-1 256 x 256 kernel where the model says its 1/128 B-per-FLOP intensity wins (problems with hundreds of such tiles:
        // the CLIP tower, few-shot prefill, lm_head forward).  M <= 64 weight-streaming shapes take the same route.
        // Problems of four and more rounds of 256 x 256 tiles, or of more than 96 tile rows (the CLIP tower at 160 images: M = 41 120),
        // keep the round-1 dispatcher below, calibrated on exactly those shapes; 2-3 rounds at moderate M (few-shot prefill, M = 4 800)
        // are ranked here, where round quantisation decides: 570 tiles are 3 rounds of the 256 x 256 kernel but 3.6 of 256 x 160
        // (measured 177 against 215 us on the QKV projection; the grid of tools/dispatch_calib.py is the evidence for both limits).
        // ragged last tile row handed to a second launch when that saves a round (big_split_rows): the costs below count the rounds of the
        // full tile rows plus ~12 us for the second launch
        const int big_rem = (a_kc && b_kc && kn.big_mode != 1 && !kn.no_row_split) ? big_split_rows(M, N) : 0;
        const float big_split_ns = big_rem ? 12000.f : 0.f;
        auto run_big = [&](const GemmParams& pp) -> int {
            if (!big_rem) return launch_big(pp, s);
            GemmParams p1 = pp;
            p1.M = M - big_rem;
            p1.tiles_m = (p1.M + BM - 1) / BM;
            const int rc1 = launch_big(p1, s);
            if (rc1) return rc1;
            const int64_t r0 = M - big_rem;
            const size_t ces = out_f32 ? 4 : 2, res_es = res_lowp ? 2 : 4;
            auto off = [](const void* base, int64_t rows, int64_t ld, size_t es) -> const void* {
                return base ? static_cast<const char*>(base) + (size_t)rows * (size_t)ld * es : nullptr;
            };
            eavqa_gemm_ln_t ln2;
            if (ln) ln2 = ln_rows_from(*ln, r0, 2);
            return gemm_impl(dtype, a_kc, b_kc, big_rem, N, K, off(A, r0, lda, 2), lda, B, ldb, const_cast<void*>(off(C, r0, ldc, ces)), ldc, out_flags,
                             alpha, bias, act, off(aux_in, r0, ld_aux, 2), const_cast<void*>(off(aux_out, r0, ld_aux, 2)), ld_aux,
                             off(residual, r0, ldr, res_es), ldr, ln ? &ln2 : nullptr, stream, 0);
        };
        int bgx, bgy;
        const int big_rounds = (big_grid((M - big_rem + GBM - 1) / GBM, (N + GBN - 1) / GBN, bgx, bgy) + 31) / 32;      // the rounds launch_big runs
        const bool many_big_tiles = big_rounds >= 4 || (big_rounds >= 2 && (M + GBM - 1) / GBM > 96);
        if (a_kc && b_kc && !kn.disable_fast && (K % 64) == 0 && kn.k64_mode != 1 && kn.shape_mode == 0 && kn.big_mode == 0 && !many_big_tiles) {
            int pick = K64_AUTO[0];
            float best_loop = 0.f;
            float best = k64_cost(p, K64_SHAPES[pick], &best_loop);
            for (int i = 1; i < N_K64_AUTO; ++i) {
                float loop;
                const float c = k64_cost(p, K64_SHAPES[K64_AUTO[i]], &loop);
                if (c < best) { best = c; pick = K64_AUTO[i]; best_loop = loop; }
            }
            // the per-row rates were calibrated on one-round problems whose operands stay in L2; a pick that needs several rounds is a
            // larger problem that re-reads its panels from the Infinity Cache / HBM: measured 1.3-1.4x slower than the model (few-shot
            // prefill: out-proj 90.8 us against 72.1 us, FFN-down 313 against 244 us on the 256 x 256 kernel) - charge it before comparing
            best += 0.35f * best_loop;
            // 256 x 256 kernel, re-fitted in round 3 on the rounds it really runs (big_grid): per round of workgroups 1.53 us per 64-deep K-tile
            // (1.38 when the whole problem is one round: panels stay in L2) + 9 us outside the K loop (first tile's round trip, C pass),
            // 3 us launch.  Fits vitL QKV / out-proj / FFN-up / FFN-down 271 / 103 / 350 / 324 against 270 / 101 / 340 / 324 us measured,
            // prefill QKV / FFN-up 214 / 214 against 191 / 203, OPT-6.7B FFN-up 217 against 211, 8192^3 822 against 851.
            const float big_cost = float(big_rounds) * (float(K / 64) * (big_rounds == 1 ? 1380.f : 1530.f) + 9000.f) + 3000.f + big_split_ns;
            if (M > 64 && big_cost < best) return run_big(p);
            return K64_SHAPES[pick].launch(p, s);
        }
        if (a_kc && b_kc && !kn.disable_fast && (K % FBK) == 0 && !ln) {      // (the round-1 BK = 32 kernels have no eavqa_gemm_ln form: the general kernel below does)
            if (kn.shape_mode >= 2 && kn.shape_mode < 7) return SHAPES[kn.shape_mode - 2].launch(p, s);
            const bool big_ok = (K % GBK) == 0 && kn.big_mode != 1;
            if (big_ok && kn.big_mode == 2) return run_big(p);
            // candidates in order of preference at equal cost: 128 x 128 (two workgroups per CU), 256 x 256, shaped tiles
            float best = tile_cost(p, 128, 128, RATE_FAST);
            int pick = -1;                                   // -1 fast, -2 big, >= 0 SHAPES[pick]
            if (big_ok && use_big(p, kn)) {
                GemmParams pf = p;
                pf.M = M - big_rem;
                best = fminf(best, tile_cost(pf, 256, 256, RATE_BIG) + big_split_ns);
                pick = -2;
            }
            if (kn.shape_mode != 1)
                for (int i = 0; i < 5; ++i) {
                    const float c = tile_cost(p, SHAPES[i].bm, SHAPES[i].bn, SHAPES[i].rate);
                    if (c < best * 0.95f) { best = c; pick = i; }
                }
            if (pick >= 0) return SHAPES[pick].launch(p, s);
            if (pick == -2) return run_big(p);
            return launch_fast(p, s, kn);
        }
        if (a_kc && b_kc) return launch(gemm_bf16_kernel<true, true>, p, s);
        if (a_kc && !b_kc) return launch(gemm_bf16_kernel<true, false>, p, s);
        if (!a_kc && b_kc) return launch(gemm_bf16_kernel<false, true>, p, s);
        return launch(gemm_bf16_kernel<false, false>, p, s);
    }
    if (a_kc && b_kc) return launch(gemm_f32_kernel<true, true>, p, s);
    if (a_kc && !b_kc) return launch(gemm_f32_kernel<true, false>, p, s);
    if (!a_kc && b_kc) return launch(gemm_f32_kernel<false, true>, p, s);
    return launch(gemm_f32_kernel<false, false>, p, s);
}
}  // namespace

extern "C" int eavqa_gemm_ex(int dtype, int a_kc, int b_kc, int M, int N, int K,
                             const void* A, int64_t lda, const void* B, int64_t ldb,
                             void* C, int64_t ldc, int out_flags, float alpha,
                             const float* bias, int act,
                             const void* aux_in, void* aux_out, int64_t ld_aux,
                             const void* residual, int64_t ldr, void* stream, int knobs) {
    return gemm_impl(dtype, a_kc, b_kc, M, N, K, A, lda, B, ldb, C, ldc, out_flags, alpha, bias, act, aux_in, aux_out, ld_aux, residual, ldr,
                     nullptr, stream, knobs);
}

extern "C" int eavqa_gemm_ln_ex(int dtype, int a_kc, int b_kc, int M, int N, int K,
                                const void* A, int64_t lda, const void* B, int64_t ldb,
                                void* C, int64_t ldc, int out_flags, float alpha,
                                const float* bias, int act,
                                const void* aux_in, void* aux_out, int64_t ld_aux,
                                const void* residual, int64_t ldr, const eavqa_gemm_ln_t* ln, void* stream, int knobs) {
    if (!ln) return EAVQA_E_ARG;
    return gemm_impl(dtype, a_kc, b_kc, M, N, K, A, lda, B, ldb, C, ldc, out_flags, alpha, bias, act, aux_in, aux_out, ld_aux, residual, ldr,
                     ln, stream, knobs);
}

extern "C" int eavqa_gemm_ln(int dtype, int a_kc, int b_kc, int M, int N, int K,
                             const void* A, int64_t lda, const void* B, int64_t ldb,
                             void* C, int64_t ldc, int out_flags, float alpha,
                             const float* bias, int act,
                             const void* aux_in, void* aux_out, int64_t ld_aux,
                             const void* residual, int64_t ldr, const eavqa_gemm_ln_t* ln, void* stream) {
    return eavqa_gemm_ln_ex(dtype, a_kc, b_kc, M, N, K, A, lda, B, ldb, C, ldc, out_flags, alpha, bias, act, aux_in, aux_out, ld_aux, residual,
                            ldr, ln, stream, 0);
}

extern "C" int eavqa_gemm(int dtype, int a_kc, int b_kc, int M, int N, int K,
                          const void* A, int64_t lda, const void* B, int64_t ldb,
                          void* C, int64_t ldc, int out_flags, float alpha,
                          const float* bias, int act,
                          const void* aux_in, void* aux_out, int64_t ld_aux,
                          const void* residual, int64_t ldr, void* stream) {
    return eavqa_gemm_ex(dtype, a_kc, b_kc, M, N, K, A, lda, B, ldb, C, ldc, out_flags, alpha, bias, act, aux_in, aux_out, ld_aux,
                         residual, ldr, stream, 0);
}

extern "C" int eavqa_gemm_pf(int dtype, int a_kc, int b_kc, int M, int N, int K,
                             const void* A, int64_t lda, const void* B, int64_t ldb,
                             void* C, int64_t ldc, int out_flags, float alpha,
                             const float* bias, int act,
                             const void* aux_in, void* aux_out, int64_t ld_aux,
                             const void* residual, int64_t ldr, void* stream, const void* next_weight, int64_t next_weight_bytes) {
    if (next_weight_bytes < 0) return EAVQA_E_ARG;
    return gemm_impl(dtype, a_kc, b_kc, M, N, K, A, lda, B, ldb, C, ldc, out_flags, alpha, bias, act, aux_in, aux_out, ld_aux, residual, ldr,
                     nullptr, stream, 0, next_weight, next_weight_bytes);
}

// ---------------------------------------------------------------------------------------------------------------- fp8 entry points
extern "C" int eavqa_quantize_rows_fp8(int dtype, int rows, int cols, const void* x, int64_t ldx, void* out, int64_t ld_out,
                                       float* row_scale, void* stream) {
    if (!x || !out || !row_scale || rows <= 0 || cols <= 0) return EAVQA_E_ARG;
    if (cols % 4) return EAVQA_E_SHAPE;
    if (ldx % 4 || ld_out % 4 || ldx < cols || ld_out < cols) return EAVQA_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(x) & 7u) || (reinterpret_cast<uintptr_t>(out) & 3u)) return EAVQA_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool reg_ok = dtype == EAVQA_BF16 && cols % 8 == 0 && cols <= 16384 && ldx % 8 == 0 && ld_out % 8 == 0 &&
                        !(reinterpret_cast<uintptr_t>(x) & 15u) && !(reinterpret_cast<uintptr_t>(out) & 7u);
    if (reg_ok) {
        const int nv = (cols / 8 + 255) / 256;
#define EAVQA_QR(NV) hipLaunchKernelGGL(quantize_rows_fp8_reg_kernel<NV>, dim3(rows), dim3(256), 0, s, cols, reinterpret_cast<const bf16_t*>(x), \
                                        ldx, reinterpret_cast<unsigned char*>(out), ld_out, row_scale)
        if (nv <= 1) EAVQA_QR(1); else if (nv <= 2) EAVQA_QR(2); else if (nv <= 4) EAVQA_QR(4); else EAVQA_QR(8);
#undef EAVQA_QR
    } else if (dtype == EAVQA_BF16)
        hipLaunchKernelGGL(quantize_rows_fp8_kernel<bf16_t>, dim3(rows), dim3(256), 0, s, cols, reinterpret_cast<const bf16_t*>(x), ldx,
                           reinterpret_cast<unsigned char*>(out), ld_out, row_scale);
    else if (dtype == EAVQA_F32)
        hipLaunchKernelGGL(quantize_rows_fp8_kernel<float>, dim3(rows), dim3(256), 0, s, cols, reinterpret_cast<const float*>(x), ldx,
                           reinterpret_cast<unsigned char*>(out), ld_out, row_scale);
    else return EAVQA_E_DTYPE;
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_gemm_fp8(int M, int N, int K, const void* A, int64_t lda, const float* a_row_scale, const void* B, int64_t ldb,
                              float b_scale, void* C, int64_t ldc, int out_f32, float alpha, const float* bias, int act,
                              const void* aux_in, void* aux_out, int64_t ld_aux, const float* residual, int64_t ldr, void* stream, int tile) {
    if (!A || !B || !C || !a_row_scale) return EAVQA_E_ARG;
    if (M <= 0 || N <= 0 || K <= 0) return EAVQA_E_ARG;
    if (act < EAVQA_ACT_NONE || act > EAVQA_ACT_QUICK_GELU) return EAVQA_E_DTYPE;
    if (K % 128) return EAVQA_E_SHAPE;
    if (lda % 16 || ldb % 16 || !eavqa_aligned16(A) || !eavqa_aligned16(B)) return EAVQA_E_ALIGN;
    if (lda < K || ldb < K || ldc < N) return EAVQA_E_ARG;
    if ((aux_in || aux_out) && ld_aux < N) return EAVQA_E_ARG;
    if (residual && ldr < N) return EAVQA_E_ARG;
    GemmParams p;
    p.A = A; p.B = B; p.C = C; p.bias = bias; p.aux_in = aux_in; p.aux_out = aux_out; p.residual = residual; p.row_scale = a_row_scale; p.ablate = 0;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ld_aux = ld_aux; p.ldr = ldr;
    p.act = act; p.out_f32 = out_f32; p.res_lowp = 0; p.out_f16 = 0; p.alpha = alpha * b_scale;
    p.group_n = 0;
    p.tiles_m = (M + BM - 1) / BM;
    p.tiles_n = (N + BN - 1) / BN;
    auto vec_ok = [](const void* ptr, int64_t ld, int bytes_per_elem) {
        return ((reinterpret_cast<uintptr_t>(ptr) % (4 * bytes_per_elem)) == 0) && (ld % 4 == 0);
    };
    p.vec_c = vec_ok(C, ldc, out_f32 ? 4 : 2);
    p.vec_aux = vec_ok(aux_in ? aux_in : aux_out, ld_aux, 2);
    p.vec_res = vec_ok(residual, ldr, 4);
    p.vec_bias = (reinterpret_cast<uintptr_t>(bias) % 16) == 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (tile > 0 && tile <= N_FP8) return FP8_SHAPES[tile - 1].launch(p, s);
    // same cost model as the bf16 specialised tiles: a stage row is 128 bytes there and here
    GemmParams q = p;
    q.K = K / 2;                                  // k64_cost counts 64-element (128-byte) steps of bf16
    int pick = 0;
    float best = k64_cost(q, FP8_SHAPES[0]);
    for (int i = 1; i < N_FP8; ++i) {
        const float c = k64_cost(q, FP8_SHAPES[i]);
        if (c < best) { best = c; pick = i; }
    }
    return FP8_SHAPES[pick].launch(p, s);
}
