// Host layer of the normalisation family (private to norm.hip's translation unit): NormCall - one call of any of the nine
// entry points, filled by field name - validate(), the float4-per-thread dispatcher and what its e4m3 forms put in front of common.h's row rule.
#pragma once
#include <type_traits>

namespace {

constexpr int LN_MAX_V4 = 32;       // row per wave, float4 per lane: cols <= 64 * 4 * 32 = 8192 in forward
constexpr int LN_MAX_V4_BWD = 16;   // 2 x 32 float4 per lane would spill: cols <= 4096 in backward
constexpr int LN_WAVES = 4;         // rows per 256-thread block
constexpr int LNS_NT = 512;         // workgroup per row (the pass over split-K partial sums)
constexpr int LNS_MAX_V4 = 8;       // float4 per thread there: cols <= 512 * 4 * 8 = 16384
constexpr int LNS_MAX_COLS = LNS_NT * 4 * LNS_MAX_V4;

enum NormKind { NORM_LAYER, NORM_RMS };                    // RMS (T5LayerNorm): no mean subtraction, no beta
enum NormPass { NORM_FWD, NORM_BWD, NORM_SPLITK };         // SPLITK: x = x_in + bias + sum of the partial sums, then the forward

// What a row-per-wave kernel is told: the fields norm_fwd_row / norm_bwd_row read, and nothing of the host's.  The kernels take them as
// plain arguments and rebuild the struct (norm.hip).
struct NormRow {
    int x_kind = 0;                         // x holds: 0 T, 1 float32, 2 bfloat16, 3 half (SPLITK: x is float32)
    int rows = 0, cols = 0;
    const void* x = nullptr; int64_t ldx = 0;
    const float* gamma = nullptr; const float* beta = nullptr; float eps = 0.f;
    void* y = nullptr; int64_t ldy = 0;
    float* mean = nullptr; float* rstd = nullptr;                               // FWD: written when non-null; BWD: read
    unsigned char* q = nullptr; int64_t ldq = 0; float* q_scale = nullptr;      // e4m3 bytes of y (FWD, SPLITK) / of dx (BWD) + one scale per row
    // BWD
    const void* dy = nullptr; int64_t lddy = 0;
    const float* dres = nullptr; float* dx = nullptr; int64_t lddx = 0;         // dres shares dx's leading dimension
    void* dx_lowp = nullptr; int64_t ld_lowp = 0;
};

// One call of an entry point: the row fields plus what only the host and the other two kernels read.
struct NormCall : NormRow {
    int kind = NORM_LAYER, pass = NORM_FWD;
    int dtype = EAVQA_BF16;                 // storage type T of y / dy / dx_lowp (the e4m3 forms round to bfloat16 before they quantise)
    bool fp8 = false;                       // the e4m3 form of the entry point: q and q_scale are required
    float* dgamma = nullptr; float* dbeta = nullptr;                            // BWD (ln_dparam_kernel)
    // SPLITK
    const float* partials = nullptr; int ks = 0; const float* bias = nullptr;
    float* x_out = nullptr; int64_t ld_out = 0;
    hipStream_t stream = nullptr;
};

// The status code of a call, in the order the entry points have always checked: arguments, shape, alignment, x_kind, dtype - and the
// backward's narrower row last; the split-K pass looks at the dtype first (after LayerNorm's beta).  Half is LayerNorm forward's alone.
inline int validate(const NormCall& c) {
    const bool layer = c.kind == NORM_LAYER, fwd = c.pass == NORM_FWD;
    const bool dtype_ok = c.dtype == EAVQA_F32 || c.dtype == EAVQA_BF16 || (c.dtype == EAVQA_F16 && layer && fwd);
    if (c.pass == NORM_SPLITK) {
        if (layer && !c.beta) return EAVQA_E_ARG;
        if (!dtype_ok) return EAVQA_E_DTYPE;
        if (!c.x || !c.gamma || (!c.y && !c.q) || c.rows <= 0 || c.cols <= 0 || c.ks < 0 || (c.ks > 0 && !c.partials)) return EAVQA_E_ARG;
        if (c.q && (!c.q_scale || c.ldq % 4)) return EAVQA_E_ARG;
        if (c.cols % 4 || c.cols > LNS_MAX_COLS) return EAVQA_E_SHAPE;
        if (c.ldx % 4 || c.ldy % 4 || (c.x_out && c.ld_out % 4)) return EAVQA_E_ALIGN;
        return EAVQA_OK;
    }
    if (!c.x || c.rows <= 0 || c.cols <= 0 || (c.fp8 ? !c.q || !c.q_scale : fwd && !c.y)) return EAVQA_E_ARG;
    if (!fwd && (!c.dy || !c.dx || !c.rstd || (layer && !c.mean))) return EAVQA_E_ARG;
    if (c.cols % 4 || (fwd && c.cols > 64 * 4 * LN_MAX_V4)) return EAVQA_E_SHAPE;
    if (c.ldx % 4 || (c.y && c.ldy % 4) || (c.q && c.ldq % 4)) return EAVQA_E_ALIGN;
    if (!fwd && (c.lddy % 4 || c.lddx % 4 || (c.dx_lowp && c.ld_lowp % 4))) return EAVQA_E_ALIGN;
    // the e4m3 forward has no `dtype` for kind 0 to mean; LayerNorm backward's x_f32 is a flag (ln_dparam_kernel reads it as one)
    if (c.x_kind < (c.fp8 && fwd ? 1 : 0) || c.x_kind > (layer && !fwd ? 1 : 3)) return EAVQA_E_DTYPE;
    if (!dtype_ok) return EAVQA_E_DTYPE;
    if (!fwd && c.cols > 64 * 4 * LN_MAX_V4_BWD) return EAVQA_E_SHAPE;
    return EAVQA_OK;
}

// f(std::integral_constant<int, NV>) for the smallest NV in {LO, 2 LO, 4 LO, ..., MAX} that holds nv float4 per thread (validate() has
// rejected a row beyond MAX).  Only the kernels of LO .. MAX are instantiated.
template <int LO, int MAX, typename F> void with_nv(int nv, F&& f) {
    if constexpr (LO < MAX)
        if (nv > LO) return with_nv<2 * LO, MAX>(nv, f);
    f(std::integral_constant<int, LO>{});
}

// The row-wise e4m3 quantisation of eavqa_quantize_rows_fp8, for a row its producer still holds in registers: the row rule of common.h
// (e4m3_row_scale, e4m3_pack4) - the same arithmetic on the same values (the row rounded to the storage type first: what that kernel
// would read back), so the bytes and the scale are those of the separate kernel.  How the row's amax is reduced (one wave, or eight through
// LDS) is the caller's.
template <typename T> __device__ __forceinline__ float4 round_to(const float4 o) {
    return make_float4((float)(T)o.x, (float)(T)o.y, (float)(T)o.z, (float)(T)o.w);
}
__device__ __forceinline__ float amax4(const float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

}  // namespace
