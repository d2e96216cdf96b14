// Host <-> kernel structs of the GEMM family (included by gemm.hip, inside its anonymous namespace): the knobs, the kernel arguments, and
// GemmCall - one call of any GEMM entry point, filled by field name.
#pragma once

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

// One call of a GEMM entry point: what the caller passed, by name.  validate() checks it, fill_params() turns it into the kernel argument,
// route() reads only its shape and knobs, rows_from() gives the same call on its last rows (gemm.hip).
struct GemmCall {
    int dtype = EAVQA_BF16;                 // element type of A / B (fp8 calls: of C / aux - their operands are e4m3 bytes, see a_row_scale)
    bool a_kc = true, b_kc = true;          // operand stored with k contiguous
    int M = 0, N = 0, K = 0;
    const void* A = nullptr; int64_t lda = 0;
    const void* B = nullptr; int64_t ldb = 0;
    void* C = nullptr; int64_t ldc = 0;
    int out_flags = 0;                      // EAVQA_GEMM_OUT_F32 | EAVQA_GEMM_RESIDUAL_LOWP | EAVQA_GEMM_STREAM_F16
    float alpha = 1.f;
    const float* bias = nullptr;
    int act = EAVQA_ACT_NONE;
    const void* aux_in = nullptr; void* aux_out = nullptr; int64_t ld_aux = 0;
    const void* residual = nullptr; int64_t ldr = 0;
    bool has_ln = false; eavqa_gemm_ln_t ln = {};     // eavqa_gemm_ln: the caller's block (held by value, so a row-shifted call owns its copy)
    const void* pf_ptr = nullptr; int64_t pf_bytes = 0;       // eavqa_gemm_pf: the look-ahead region
    const float* a_row_scale = nullptr; float b_scale = 1.f;  // eavqa_gemm_fp8 (a_row_scale non-null marks the call as fp8): dequantisation scales
    hipStream_t stream = nullptr;
    Knobs knobs;
};
