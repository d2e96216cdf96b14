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
//
// This file holds no kernel: it is the host layer - validate(), fill_params(), route(), run(), rows_from() and the entry points - over
//   gemm_params.h      knobs, kernel arguments, GemmCall (the dynamic-LDS opt-in is common.h's)
//   gemm_general.hip   tile map, eavqa_gemm_ln row statistics, the shared epilogue; the register-staged bf16 / f32 kernels
//   gemm_r1.hip        round-1 LDS-DMA family: 128 x 128 fast, shaped tiles, 256 x 256; grid planners, tile_cost, use_big, big_split_rows
//   gemm_k64.hip       full-line (BK = 64) loader / consumer tiles, K64_SHAPES, k64_cost, argmin_cost
//   gemm_fp8.hip       fp8 tiles and the row quantisation kernels
//   gemm_skinny.hip    M <= 64 weight-streaming kernel
// all one translation unit, in dependency order, inside one anonymous namespace.
#include "common.h"

namespace {
#include "gemm_params.h"
#include "gemm_general.hip"
#include "gemm_r1.hip"
#include "gemm_k64.hip"
#include "gemm_fp8.hip"
#include "gemm_skinny.hip"

// ------------------------------------------------------------------------------------------------------------------------ validate
// The order of the checks decides the code a call with two faults gets: tests/test_abi.py (GEMM_REJECTIONS) pins it.
int validate(const GemmCall& c) {
    const bool fp8 = c.a_row_scale != nullptr;
    if (c.has_ln) {
        const eavqa_gemm_ln_t& ln = c.ln;
        const bool ln_consumer = ln.ln_stats != nullptr;
        if (ln.copy_out && ln.ld_copy < c.N) return EAVQA_E_ARG;
        if (ln.stats_out && ln.stats_ld < (c.N + 63) / 64) return EAVQA_E_ARG;
        if (ln_consumer && (!ln.ln_c || ln.ln_parts <= 0 || ln.ln_ld < ln.ln_parts || ln.ln_cols <= 0 || !(ln.ln_eps >= 0.f))) return EAVQA_E_ARG;
        if ((ln.mean_out != nullptr) != (ln.rstd_out != nullptr) || (ln.mean_out && !ln_consumer)) return EAVQA_E_ARG;
        if (!(c.a_kc && c.b_kc)) return EAVQA_E_SHAPE;      // the eavqa_gemm_ln form exists for k-contiguous operands (the frozen LM's Linear layers)
    }
    if (c.out_flags & ~(EAVQA_GEMM_OUT_F32 | EAVQA_GEMM_RESIDUAL_LOWP | EAVQA_GEMM_STREAM_F16)) return EAVQA_E_ARG;
    if ((c.out_flags & (EAVQA_GEMM_RESIDUAL_LOWP | EAVQA_GEMM_STREAM_F16)) && c.dtype != EAVQA_BF16) return EAVQA_E_DTYPE;   // 16-bit streams: bf16 operands only
    if (!c.A || !c.B || !c.C) return EAVQA_E_ARG;
    if (c.M <= 0 || c.N <= 0 || c.K <= 0) return EAVQA_E_ARG;
    if (c.dtype != EAVQA_F32 && c.dtype != EAVQA_BF16) return EAVQA_E_DTYPE;
    if (c.act < EAVQA_ACT_NONE || c.act > EAVQA_ACT_QUICK_GELU) return EAVQA_E_DTYPE;
    // the contiguous memory dimension of each operand is read in 16-byte chunks; the fp8 tiles step through K 128 at a time (this check
    // is the fp8 entry point's alone, but its place among the others is part of the pinned order)
    const int vec = fp8 ? 16 : c.dtype == EAVQA_BF16 ? 8 : 4;
    const int a_contig = c.a_kc ? c.K : c.M, b_contig = c.b_kc ? c.K : c.N;
    if (a_contig % vec || b_contig % vec || (fp8 && c.K % 128)) return EAVQA_E_SHAPE;
    if (c.lda % vec || c.ldb % vec) return EAVQA_E_ALIGN;
    if (!eavqa_aligned16(c.A) || !eavqa_aligned16(c.B)) return EAVQA_E_ALIGN;
    if (c.lda < a_contig || c.ldb < b_contig || c.ldc < c.N) return EAVQA_E_ARG;
    if ((c.aux_in || c.aux_out) && c.ld_aux < c.N) return EAVQA_E_ARG;
    if (c.residual && c.ldr < c.N) return EAVQA_E_ARG;
    return EAVQA_OK;
}

// 16-byte (8-byte for 16-bit elements) vector access allowed on a matrix of the epilogue
bool vec_ok(const void* ptr, int64_t ld, int bytes_per_elem) {
    return ((reinterpret_cast<uintptr_t>(ptr) % (4 * bytes_per_elem)) == 0) && (ld % 4 == 0);
}

// --------------------------------------------------------------------------------------------------------------------- fill_params
// The kernel argument of a validated call.
void fill_params(const GemmCall& c, GemmParams& p) {
    const Knobs& kn = c.knobs;
    const bool fp8 = c.a_row_scale != nullptr;
    const int out_f32 = c.out_flags & EAVQA_GEMM_OUT_F32;
    const int stream_f16 = (c.out_flags & EAVQA_GEMM_STREAM_F16) != 0;
    const int res_lowp = (c.out_flags & EAVQA_GEMM_RESIDUAL_LOWP) ? (stream_f16 ? 2 : 1) : 0;
    p.A = c.A; p.B = c.B; p.C = c.C; p.bias = c.bias; p.aux_in = c.aux_in; p.aux_out = c.aux_out; p.residual = c.residual;
    p.row_scale = c.a_row_scale; p.ablate = kn.ablate;
    p.M = c.M; p.N = c.N; p.K = c.K; p.lda = c.lda; p.ldb = c.ldb; p.ldc = c.ldc; p.ld_aux = c.ld_aux; p.ldr = c.ldr;
    p.act = c.act; p.out_f32 = out_f32; p.res_lowp = res_lowp; p.out_f16 = stream_f16 && !out_f32; p.alpha = c.alpha * c.b_scale;
    p.group_n = fp8 ? 0 : kn.group_n == 0 ? BIG_GROUP_N : kn.group_n - 1;      // (read by the 256 x 256 kernel only)
    p.tiles_m = (c.M + BM - 1) / BM;
    p.tiles_n = (c.N + BN - 1) / BN;
    const int esz = c.dtype == EAVQA_BF16 ? 2 : 4;
    p.vec_c = vec_ok(c.C, c.ldc, out_f32 ? 4 : esz);
    p.vec_aux = vec_ok(c.aux_in ? c.aux_in : c.aux_out, c.ld_aux, esz);
    p.vec_res = vec_ok(c.residual, c.ldr, res_lowp ? esz : 4);
    p.vec_bias = (reinterpret_cast<uintptr_t>(c.bias) % 16) == 0;
    if (c.has_ln) {
        const eavqa_gemm_ln_t& ln = c.ln;
        p.copy_out = ln.copy_out; p.ld_copy = ln.ld_copy; p.vec_copy = ln.copy_out ? vec_ok(ln.copy_out, ln.ld_copy, esz) : 0;
        p.stats_out = ln.stats_out; p.stats_ld = ln.stats_ld;
        if (ln.ln_stats) {
            p.ln_stats = ln.ln_stats; p.ln_parts = ln.ln_parts; p.ln_ld = ln.ln_ld; p.ln_c = ln.ln_c;
            p.ln_inv_n = 1.0f / float(ln.ln_cols); p.ln_eps = ln.ln_eps; p.mean_out = ln.mean_out; p.rstd_out = ln.rstd_out;
        }
    }
    // the look-ahead region: honoured by the full-line tiles the dispatcher picks from, ignored (correct, only cold) by every other kernel
    if (c.pf_ptr && c.pf_bytes > 0 && !c.has_ln) { p.pf_ptr = c.pf_ptr; p.pf_bytes = c.pf_bytes; }
}

// --------------------------------------------------------------------------------------------------------------------------- route
// Which kernel a shape gets: a pure function of the shape and the knobs (no HIP call, no pointer), exported for the tests as
// eavqa_gemm_route (include/eavqa_test.h numbers Kind the same way).
enum class Kind { F32General, General, Skinny, Fast, Shaped, Big, K64 };
struct Route {
    Kind kind;
    int index;          // K64: entry of K64_SHAPES; Shaped: entry of SHAPES; General / F32General: operand layout, 2 * !a_kc + !b_kc; else 0
    int split_rows;     // Big: the last rows (M % 256 of them) go to a second launch, routed on their own with knobs 0; else 0
};

Route route(int dtype, bool a_kc, bool b_kc, int M, int N, int K, bool has_ln, const Knobs& kn) {
    const int layout = 2 * !a_kc + !b_kc;
    if (dtype != EAVQA_BF16) return {Kind::F32General, layout, 0};
    const bool kc = a_kc && b_kc;
    const bool k64 = kc && (K % 64) == 0;                                     // operands the full-line tiles and the 256 x 256 kernel take
    const bool r1 = kc && !kn.disable_fast && (K % FBK) == 0 && !has_ln;      // ... and the round-1 BK = 32 kernels (they have no eavqa_gemm_ln form: the general kernel has)
    // M <= 64 with few columns (T5 decoder passes at one or two tokens: N = 2048 is 26 tiles of 128 x 80 for 256 CUs): the 16-column
    // weight-streaming kernel has N / 16 workgroups - 8.7 against 15.1 us at N = K = 2048, 20.9 against 31.9 us at K = 5120 (cold
    // weights); from N = 6144 on the tiles win again (16.6 against 22.3 us at N = 10240)
    const bool few_columns = kn.k64_mode == 0 && kn.shape_mode == 0 && kn.big_mode == 0 && N <= 4096;
    const bool skinny = r1 && M <= 64 && N >= 64 && (kn.k64_mode == 1 || (K % 64) != 0 || few_columns);
    // ragged last tile row of the 256 x 256 kernel handed to a second launch when that saves a round (big_split_rows)
    const auto big_split = [&] { return (kc && kn.big_mode != 1 && !kn.no_row_split) ? big_split_rows(M, N) : 0; };

    // ---- selections forced by a knob (eavqa_gemm_ex; the production rule is the rest of the function)
    if (k64 && kn.k64_mode >= 2 && kn.k64_mode < 2 + N_K64) return {Kind::K64, kn.k64_mode - 2, 0};
    if (r1 && !skinny) {      // (a forced round-1 kernel yields to the M <= 64 kernel where that one is the only specialised kernel left)
        if (kn.shape_mode >= 2 && kn.shape_mode < 7) return {Kind::Shaped, kn.shape_mode - 2, 0};
        if (k64 && kn.big_mode == 2) return {Kind::Big, 0, big_split()};
    }

    // ---- the rule.  Knobs only take candidates away: disable_fast every specialised kernel, k64_mode 1 the full-line tiles, any shape_mode /
    // big_mode the full-line tiles too (they choose among the round-1 kernels), shape_mode 1 the shaped tiles, big_mode 1 the 256 x 256 kernel,
    // no_row_split its second launch.
    if (skinny) return {Kind::Skinny, 0, 0};
    // the costs below count the rounds of the full tile rows of a row-split problem plus ~12 us for its second launch
    const int big_rem = big_split();
    const float big_split_ns = big_rem ? 12000.f : 0.f;
    // Default dispatch (K % 64 == 0): the loader / consumer specialised full-line tile the cost model ranks first, or the
    // round-1 256 x 256 kernel where the model says its 1/128 B-per-FLOP intensity wins (problems with hundreds of such tiles:
    // the CLIP tower, few-shot prefill, lm_head forward).  M <= 64 weight-streaming shapes take the same route.
    // Problems of four and more rounds of 256 x 256 tiles, or of more than 96 tile rows (the CLIP tower at 160 images: M = 41 120),
    // keep the round-1 dispatcher below, calibrated on exactly those shapes; 2-3 rounds at moderate M (few-shot prefill, M = 4 800)
    // are ranked here, where round quantisation decides: 570 tiles are 3 rounds of the 256 x 256 kernel but 3.6 of 256 x 160
    // (measured 177 against 215 us on the QKV projection; the grid of tools/dispatch_calib.py is the evidence for both limits).
    int bgx, bgy;
    const int big_rounds = (big_grid((M - big_rem + GBM - 1) / GBM, (N + GBN - 1) / GBN, bgx, bgy) + 31) / 32;      // the rounds launch_big runs
    const bool many_big_tiles = big_rounds >= 4 || (big_rounds >= 2 && (M + GBM - 1) / GBM > 96);
    const bool full_line = k64 && !kn.disable_fast && kn.k64_mode != 1 && kn.shape_mode == 0 && kn.big_mode == 0;
    if (full_line && !many_big_tiles) {
        float best, best_loop;
        const int pick = argmin_cost(M, N, K, K64_SHAPES, K64_AUTO, N_K64_AUTO, &best, &best_loop);
        // the per-row rates were calibrated on one-round problems whose operands stay in L2; a pick that needs several rounds is a
        // larger problem that re-reads its panels from the Infinity Cache / HBM: measured 1.3-1.4x slower than the model (few-shot
        // prefill: out-proj 90.8 us against 72.1 us, FFN-down 313 against 244 us on the 256 x 256 kernel) - charge it before comparing
        best += 0.35f * best_loop;
        // 256 x 256 kernel, re-fitted in round 3 on the rounds it really runs (big_grid): per round of workgroups 1.53 us per 64-deep K-tile
        // (1.38 when the whole problem is one round: panels stay in L2) + 9 us outside the K loop (first tile's round trip, C pass),
        // 3 us launch.  Fits vitL QKV / out-proj / FFN-up / FFN-down 271 / 103 / 350 / 324 against 270 / 101 / 340 / 324 us measured,
        // prefill QKV / FFN-up 214 / 214 against 191 / 203, OPT-6.7B FFN-up 217 against 211, 8192^3 822 against 851.
        const float big_cost = float(big_rounds) * (float(K / 64) * (big_rounds == 1 ? 1380.f : 1530.f) + 9000.f) + 3000.f + big_split_ns;
        if (M > 64 && big_cost < best) return {Kind::Big, 0, big_rem};
        return {Kind::K64, pick, 0};
    }
    if (r1) {
        // candidates in order of preference at equal cost: 128 x 128 (two workgroups per CU), 256 x 256, shaped tiles
        float best = tile_cost(M, N, K, 128, 128, RATE_FAST);
        Route pick = {Kind::Fast, 0, 0};
        if (k64 && use_big(M, N, K, kn)) {               // (once it is a candidate the 256 x 256 kernel displaces the 128 x 128 one whatever their costs)
            best = fminf(best, tile_cost(M - big_rem, N, K, 256, 256, RATE_BIG) + big_split_ns);
            pick = {Kind::Big, 0, big_rem};
        }
        if (kn.shape_mode != 1)
            for (int i = 0; i < 5; ++i) {
                const float c = tile_cost(M, N, K, SHAPES[i].bm, SHAPES[i].bn, SHAPES[i].rate);
                if (c < best * 0.95f) { best = c; pick = {Kind::Shaped, i, 0}; }
            }
        return pick;
    }
    return {Kind::General, layout, 0};
}

// ----------------------------------------------------------------------------------------------------------------------------- run
// The launch of a routed call: the only place that names the launchers.
int run(const Route& r, const GemmParams& p, hipStream_t s, const Knobs& kn) {
    switch (r.kind) {
        case Kind::K64: return K64_SHAPES[r.index].launch(p, s);
        case Kind::Shaped: return SHAPES[r.index].launch(p, s);
        case Kind::Skinny: return launch_skinny(p, s);
        case Kind::Big: return launch_big(p, s);
        case Kind::Fast: return launch_fast(p, s, kn);
        case Kind::General:
            switch (r.index) {
                case 0: return launch_general<gemm_bf16_kernel<true, true>>(p, s);
                case 1: return launch_general<gemm_bf16_kernel<true, false>>(p, s);
                case 2: return launch_general<gemm_bf16_kernel<false, true>>(p, s);
                default: return launch_general<gemm_bf16_kernel<false, false>>(p, s);
            }
        case Kind::F32General:
            switch (r.index) {
                case 0: return launch_general<gemm_f32_kernel<true, true>>(p, s);
                case 1: return launch_general<gemm_f32_kernel<true, false>>(p, s);
                case 2: return launch_general<gemm_f32_kernel<false, true>>(p, s);
                default: return launch_general<gemm_f32_kernel<false, false>>(p, s);
            }
    }
    return EAVQA_E_ARG;
}

// Rows [r0, M) of a call: every row-indexed pointer advanced, the eavqa_gemm_ln block's included.  The second launch of a row-split problem
// runs it as a call of its own: library-default knobs and no look-ahead region.
GemmCall rows_from(const GemmCall& c, int64_t r0) {
    const size_t esz = c.dtype == EAVQA_BF16 ? 2 : 4;
    const size_t c_es = (c.out_flags & EAVQA_GEMM_OUT_F32) ? 4 : esz, res_es = (c.out_flags & EAVQA_GEMM_RESIDUAL_LOWP) ? esz : 4;
    auto off = [r0](auto* base, int64_t ld, size_t es) {         // null stays null
        return base ? reinterpret_cast<decltype(base)>(reinterpret_cast<uintptr_t>(base) + (size_t)r0 * (size_t)ld * es) : nullptr;
    };
    GemmCall y = c;
    y.M = c.M - int(r0);
    y.A = off(c.A, c.a_kc ? c.lda : 1, esz);
    y.C = off(c.C, c.ldc, c_es);
    y.aux_in = off(c.aux_in, c.ld_aux, esz); y.aux_out = off(c.aux_out, c.ld_aux, esz);
    y.residual = off(c.residual, c.ldr, res_es);
    if (c.has_ln) {
        y.ln.copy_out = off(c.ln.copy_out, c.ln.ld_copy, esz);
        y.ln.stats_out = off(c.ln.stats_out, c.ln.stats_ld, 2 * sizeof(float));
        y.ln.ln_stats = off(c.ln.ln_stats, c.ln.ln_ld, 2 * sizeof(float));
        y.ln.mean_out = off(c.ln.mean_out, 1, sizeof(float));
        y.ln.rstd_out = off(c.ln.rstd_out, 1, sizeof(float));
    }
    y.pf_ptr = nullptr; y.pf_bytes = 0;
    y.knobs = Knobs(0);
    return y;
}

// every bf16 / f32 entry point: validate, fill, route, run - a row-split problem as two calls
int gemm(const GemmCall& c) {
    if (const int rc = validate(c)) return rc;
    GemmParams p;
    fill_params(c, p);
    const Route r = route(c.dtype, c.a_kc, c.b_kc, c.M, c.N, c.K, c.has_ln, c.knobs);
    if (r.split_rows == 0) return run(r, p, c.stream, c.knobs);
    p.M = c.M - r.split_rows;
    p.tiles_m = (p.M + BM - 1) / BM;
    if (const int rc = run(r, p, c.stream, c.knobs)) return rc;
    return gemm(rows_from(c, c.M - r.split_rows));
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------- entry points
// Each one: the check that is its own alone, a GemmCall filled by name, one call.  The arguments the five bf16 / f32 forms share go into
// the fields of the same names:
#define EAVQA_GEMM_ARGS                                                                                                          \
    int dtype, int a_kc, int b_kc, int M, int N, int K, const void *A, int64_t lda, const void *B, int64_t ldb, void *C, int64_t ldc, \
        int out_flags, float alpha, const float *bias, int act, const void *aux_in, void *aux_out, int64_t ld_aux,               \
        const void *residual, int64_t ldr
#define EAVQA_GEMM_CALL(c)                                                                                                       \
    GemmCall c;                                                                                                                  \
    c.dtype = dtype; c.a_kc = a_kc != 0; c.b_kc = b_kc != 0; c.M = M; c.N = N; c.K = K;                                          \
    c.A = A; c.lda = lda; c.B = B; c.ldb = ldb; c.C = C; c.ldc = ldc;                                                            \
    c.out_flags = out_flags; c.alpha = alpha; c.bias = bias; c.act = act;                                                        \
    c.aux_in = aux_in; c.aux_out = aux_out; c.ld_aux = ld_aux; c.residual = residual; c.ldr = ldr;                               \
    c.stream = reinterpret_cast<hipStream_t>(stream)

extern "C" int eavqa_gemm(EAVQA_GEMM_ARGS, void* stream) {
    EAVQA_GEMM_CALL(c);
    return gemm(c);
}

extern "C" int eavqa_gemm_ex(EAVQA_GEMM_ARGS, void* stream, int knobs) {
    EAVQA_GEMM_CALL(c);
    c.knobs = Knobs(knobs);
    return gemm(c);
}

extern "C" int eavqa_gemm_ln_ex(EAVQA_GEMM_ARGS, const eavqa_gemm_ln_t* ln, void* stream, int knobs) {
    if (!ln) return EAVQA_E_ARG;
    EAVQA_GEMM_CALL(c);
    c.has_ln = true; c.ln = *ln;
    c.knobs = Knobs(knobs);
    return gemm(c);
}

extern "C" int eavqa_gemm_ln(EAVQA_GEMM_ARGS, const eavqa_gemm_ln_t* ln, void* stream) {
    if (!ln) return EAVQA_E_ARG;
    EAVQA_GEMM_CALL(c);
    c.has_ln = true; c.ln = *ln;
    return gemm(c);
}

extern "C" int eavqa_gemm_pf(EAVQA_GEMM_ARGS, void* stream, const void* next_weight, int64_t next_weight_bytes) {
    if (next_weight_bytes < 0) return EAVQA_E_ARG;
    EAVQA_GEMM_CALL(c);
    c.pf_ptr = next_weight; c.pf_bytes = next_weight_bytes;
    return gemm(c);
}
#undef EAVQA_GEMM_CALL
#undef EAVQA_GEMM_ARGS

// The route of a shape, for the tests (include/eavqa_test.h): validate() on a call of that shape whose pointers and leading dimensions are
// in order, then route().
extern "C" int eavqa_gemm_route(int dtype, int a_kc, int b_kc, int M, int N, int K, int has_ln, int knobs, int* split_rows) {
    GemmCall c;
    c.dtype = dtype; c.a_kc = a_kc != 0; c.b_kc = b_kc != 0; c.M = M; c.N = N; c.K = K; c.has_ln = has_ln != 0; c.knobs = Knobs(knobs);
    c.A = c.B = c.C = reinterpret_cast<void*>(uintptr_t(16));     // (aligned, never dereferenced)
    c.lda = a_kc ? K : M; c.ldb = b_kc ? K : N; c.ldc = N;
    if (const int rc = validate(c)) return rc;
    const Route r = route(c.dtype, c.a_kc, c.b_kc, M, N, K, c.has_ln, c.knobs);
    if (split_rows) *split_rows = r.split_rows;
    return int(r.kind) * 256 + r.index;
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
    if (!a_row_scale) return EAVQA_E_ARG;
    GemmCall c;                                     // (dtype: C and aux are bf16 unless out_f32; the operands are e4m3 bytes, k contiguous)
    c.M = M; c.N = N; c.K = K; c.A = A; c.lda = lda; c.a_row_scale = a_row_scale; c.B = B; c.ldb = ldb; c.b_scale = b_scale;
    c.C = C; c.ldc = ldc; c.out_flags = out_f32 ? EAVQA_GEMM_OUT_F32 : 0; c.alpha = alpha; c.bias = bias; c.act = act;
    c.aux_in = aux_in; c.aux_out = aux_out; c.ld_aux = ld_aux; c.residual = residual; c.ldr = ldr;
    c.stream = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = validate(c)) return rc;
    GemmParams p;
    fill_params(c, p);
    if (tile > 0 && tile <= N_FP8) return FP8_SHAPES[tile - 1].launch(p, c.stream);
    // same cost model as the bf16 specialised tiles: a stage row is 128 bytes there and here (k64_cost counts 64-element steps of bf16)
    float best;
    return FP8_SHAPES[argmin_cost(M, N, K / 2, FP8_SHAPES, nullptr, N_FP8, &best)].launch(p, c.stream);
}
