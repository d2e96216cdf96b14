// Host layer of the decode-step kernels (private to the library; decode.hip, decode_direct.hip, attention_decode.hip): per family
// validate() - the status code of a call, in the order the entry points have always checked - and a PLAN, a pure function from shape and
// selector to (variant, grid, workgroup, LDS bytes) that the host-only eavqa_*_route entry points report (tests/test_decode_route_cpu.py
// pins it).  Each kernel file adds the dispatcher from a plan's variant to an instantiation and one launcher: validate -> plan -> opt-in
// -> fill args -> launch.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int DECODE_LDS_MAX = 150 * 1024;      // what the decode kernels opt into; a plan beyond it is EAVQA_E_SHAPE

inline int rows_mf(int M) { return M <= 16 ? 1 : (M <= 32 ? 2 : 4); }      // 16-row fragments that hold M <= 64 rows

// one destination column segment of a finish / direct-GEMM epilogue (a by-value kernel argument)
struct FinishSeg { void* dst; int64_t ld; };

// ---- naming an instantiation: with_value<Vs...>(v, f) calls f(std::integral_constant<int, V>) for the V that equals v, and a dispatcher
// hands its launcher KernelTag<kernel>.  Both answer false when nothing matched: the plan named a variant that is not instantiated.
template <int V> using Int = std::integral_constant<int, V>;
template <auto Kernel> struct KernelTag { static constexpr auto value = Kernel; };
template <int... Vs, typename F> bool with_value(int v, F&& f) { return ((v == Vs && f(Int<Vs>{})) || ...); }

// ------------------------------------------------------------------------------------------------------------------- split-K GEMM
// One call of eavqa_gemm_splitk / _ex / eavqa_gemm_fp8_splitk.  a_row_scale non-null marks the call as fp8 (as in GemmCall): A and B are
// e4m3 bytes, a k-step is 128 values instead of 32 - a 16-byte piece holds 16 values instead of 8 - and every rule below is the bf16 rule in bytes.
struct SplitKCall {
    int dtype = EAVQA_BF16, M = 0, N = 0, K = 0;
    const void* A = nullptr; int64_t lda = 0; const void* B = nullptr; int64_t ldb = 0;
    const float* a_row_scale = nullptr; float b_scale = 1.f;
    float* partials = nullptr; int ks = 0;
    hipStream_t stream = nullptr;
    int sel = 0;        // eavqa_gemm_splitk_ex: bits [7:0] U, [11:8] NW, [15:12] NF; a zero field = the default
};
struct SplitKPlan { int mf, nf, nw, u; dim3 grid; int block; int lds; };

inline int validate(const SplitKCall& c) {
    const bool fp8 = c.a_row_scale != nullptr;
    const int kstep = fp8 ? 128 : 32, piece = fp8 ? 16 : 8;
    if (c.dtype != EAVQA_BF16) return EAVQA_E_DTYPE;
    if (!c.A || !c.B || !c.partials || c.M <= 0 || c.M > 64 || c.N <= 0 || c.K <= 0 || c.ks <= 0) return EAVQA_E_ARG;
    if (c.K % (kstep * c.ks) || c.lda < c.K || c.ldb < c.K) return EAVQA_E_SHAPE;
    if (c.lda % piece || c.ldb % piece || !eavqa_aligned16(c.A) || !eavqa_aligned16(c.B)) return EAVQA_E_ALIGN;
    return EAVQA_OK;
}

// Recommended split (measured on OPT-2.7B's four decode shapes at M = 32, tools/decode_bench.py --sweep, profiles/round2_decode.md): 8-wave
// workgroups of 128 columns (the A slice is staged once per 128 columns: a quarter of a byte of A per weight byte), ONE workgroup per
// CU where the shape allows it - the largest ks with (N / 128) x ks <= 256 and slices of at least 512 bytes per row - and a deep
// weight-load window when the slice has 1024+ bytes per row.  The staged A slice stays <= 64 KiB.  0: the shape is not supported.
inline int splitk_ks(bool fp8, int M, int N, int K) {
    const int kstep = fp8 ? 128 : 32, bytes = fp8 ? 1 : 2;
    if (M <= 0 || M > 64 || N <= 0 || K <= 0 || K % kstep) return 0;
    const int mf = rows_mf(M), groups = (N + 127) / 128;
    int best = 0, one_round = 0, fine = 0;
    for (int ks = 1; ks <= 32; ++ks) {
        if (K % (kstep * ks)) continue;
        const int KS = K / ks;
        if (KS * mf * 16 * bytes > 64 * 1024) continue;      // staged A slice
        if (!best) best = ks;                                // smallest admissible split
        if (groups * ks <= 256 && KS * bytes >= 512) one_round = ks;
        if (KS * bytes >= 1024) fine = ks;
    }
    // no split fits one workgroup per CU (FFN-up of OPT-2.7B: 80 column groups, K = 2560 admits ks >= 4): several workgroups share a CU
    // anyway, and slices of 1024 bytes balance better than the smallest split (round-3 sweep: ks = 5 15.4 us against ks = 4 17.7 us)
    return one_round ? one_round : (fine > best ? fine : best);
}

// the instantiated (MF, NF, NW, U): bf16 {1, 2, 4} x {1, 2} x {4, 8} x {8, 16}; fp8 {1, 2, 4} x 1 x 8 x {4, 8}
constexpr bool splitk_instantiated(bool fp8, int nf, int nw, int u) {
    return fp8 ? nf == 1 && nw == 8 && (u == 4 || u == 8) : (nf == 1 || nf == 2) && (nw == 4 || nw == 8) && (u == 8 || u == 16);
}

// of a call validate() accepted.  The window holds 1024 bytes per weight row when the slice has as many (16 k-steps of bf16, 8 of e4m3:
// the same 16 loads per lane), else 512.
inline int splitk_plan(const SplitKCall& c, SplitKPlan& p) {
    const bool fp8 = c.a_row_scale != nullptr;
    const int kstep = fp8 ? 128 : 32, bytes = fp8 ? 1 : 2, KS = c.K / c.ks;
    p.mf = rows_mf(c.M);
    p.lds = KS * p.mf * 16 * bytes;
    if (p.lds > DECODE_LDS_MAX) return EAVQA_E_SHAPE;
    p.u = (c.sel & 0xFF) ? (c.sel & 0xFF) : (KS * bytes >= 1024 ? 1024 : 512) / (kstep * bytes);
    p.nw = ((c.sel >> 8) & 0xF) ? ((c.sel >> 8) & 0xF) : 8;
    p.nf = ((c.sel >> 12) & 0xF) ? ((c.sel >> 12) & 0xF) : 1;
    if (!splitk_instantiated(fp8, p.nf, p.nw, p.u)) return EAVQA_E_ARG;
    const int cols = 16 * p.nf * p.nw;
    p.grid = dim3((c.N + cols - 1) / cols, c.ks);
    p.block = 64 * p.nw;
    return EAVQA_OK;
}

// ------------------------------------------------------------------------------------------------------------------- direct GEMM
constexpr unsigned DIRECT_OOB = 0x80000000u;    // A and B are read through buffer descriptors: their extents stay below 2 GB

// the instantiated (MF, NF, AF32): 64 rows take at most 2 fragments, and the fp32-A kernels beyond these spill (tools/kernel_regs.sh)
constexpr bool direct_instantiated(int mf, int nf, bool af32) {
    return (mf == 1 || mf == 2 || mf == 4) && nf >= 1 && nf <= (mf == 4 ? 2 : 4) && (!af32 || (mf <= 2 && nf <= 3 + (mf == 1)));
}

struct DirectPlan { int mf, nf; bool af32, nt; int row_groups, out_cols; dim3 grid; int lds; };

inline int validate(const eavqa_decode_gemm_t& a) {
    if (!a.A || !a.B || !a.out[0]) return EAVQA_E_ARG;
    const int M = a.M, N = a.N, K = a.K;
    if (M <= 0 || M > 64 || N <= 0 || K <= 0) return EAVQA_E_ARG;
    if (K % 64) return EAVQA_E_SHAPE;
    if (a.a_kind < 0 || a.a_kind > 2) return EAVQA_E_DTYPE;
    if (a.act < EAVQA_ACT_NONE || a.act > EAVQA_ACT_QUICK_GELU) return EAVQA_E_DTYPE;
    const bool af32 = a.a_kind != 0;
    if (af32 && (!a.gamma || !a.stats_in || a.n_stats_in <= 0 || a.n_stats_in > 256 || a.stats_in_cols <= 0 || K > 16384)) return EAVQA_E_ARG;
    // the partials must cover the row, and every one of them must begin inside it: the kernel takes min(stats_in_cols, K - i stats_in_cols)
    // as the count of partial i, and a negative count corrupts the running count of the row's statistics
    if (af32 && (int64_t)a.n_stats_in * a.stats_in_cols < K) return EAVQA_E_ARG;
    if (af32 && (int64_t)(a.n_stats_in - 1) * a.stats_in_cols >= K) return EAVQA_E_ARG;
    if (a.lda < K || a.ldb < K || a.lda % (af32 ? 4 : 8) || a.ldb % 8) return EAVQA_E_ALIGN;
    if (!eavqa_aligned16(a.A) || !eavqa_aligned16(a.B) || (af32 && (!eavqa_aligned16(a.gamma) || (a.beta && !eavqa_aligned16(a.beta)))))
        return EAVQA_E_ALIGN;
    if (a.n_seg < 1 || a.n_seg > 3 || N % a.n_seg) return EAVQA_E_SHAPE;
    for (int i = 1; i < a.n_seg; ++i)
        if (!a.out[i]) return EAVQA_E_ARG;
    if (a.gated_rows && a.gated_rows < N) return EAVQA_E_ARG;
    return EAVQA_OK;
}

// bytes A and B span, for the buffer descriptors
inline int direct_extents(int M, int N, int K, int64_t lda, int64_t ldb, bool af32, int gated_rows, unsigned& a_bytes, unsigned& b_bytes) {
    const int64_t b_rows = gated_rows ? (int64_t)gated_rows + N : N;
    const int64_t bb = ((b_rows - 1) * ldb + K) * 2, ab = ((int64_t)(M - 1) * lda + K) * (af32 ? 4 : 2);
    if (bb >= (int64_t)DIRECT_OOB || ab >= (int64_t)DIRECT_OOB) return EAVQA_E_SHAPE;
    a_bytes = (unsigned)ab; b_bytes = (unsigned)bb;
    return EAVQA_OK;
}

// Of a shape validate() accepted.  Columns of C per workgroup: the fewest 16-column fragments that bring the grid down to one round of 256
// workgroups; a gated workgroup holds both halves of its columns, so its NF is even.  The fp32-A kernels hold 16 raw floats per row
// fragment and k-block: 64 rows run as two row groups of 32, and 3 fragments is their limit.
// sel (include/eavqa_test.h): bits [3:0] force NF, bit 4 = plain (not non-temporal) weight loads, bits [11:8] row groups.
inline int direct_plan(int M, int N, int K, int a_kind, bool gated, int sel, DirectPlan& p) {
    const int mf = rows_mf(M), frags = (N + 15) / 16;
    p.af32 = a_kind != 0;
    p.nt = !(sel & 0x10);
    const int max_nf = (mf == 4 && !p.af32) ? 2 : (p.af32 ? 3 : 4);
    if (sel & 0xF) p.nf = sel & 0xF;
    else if (gated) p.nf = (frags <= 256 || max_nf < 4) ? 2 : 4;
    else p.nf = (frags + 255) / 256 > max_nf ? max_nf : (frags + 255) / 256;
    if (gated && (p.nf & 1)) return EAVQA_E_ARG;
    p.mf = mf; p.row_groups = 1;
    if (p.af32 && mf == 4) { p.mf = 2; p.row_groups = 2; }
    if ((sel >> 8) & 0xF) {                                         // split the rows over several workgroups (A / B measurements)
        p.row_groups = (sel >> 8) & 0xF;
        p.mf = rows_mf((M + p.row_groups - 1) / p.row_groups);
    }
    if (!direct_instantiated(p.mf, p.nf, p.af32)) return EAVQA_E_SHAPE;
    // LDS: the 8 accumulator slabs + one output tile; before them (fp32 A) gamma, beta and the rows' statistics
    const size_t rows = 16 * p.mf, cols = 16 * p.nf;
    const size_t epi = (8 * rows * (cols + 4) + rows * (cols + 1)) * 4, pre = p.af32 ? ((size_t)2 * K + 128) * 4 : 0;
    if ((epi > pre ? epi : pre) > (size_t)DECODE_LDS_MAX) return EAVQA_E_SHAPE;
    p.lds = (int)(epi > pre ? epi : pre);
    p.out_cols = gated ? 8 * p.nf : 16 * p.nf;
    p.grid = dim3((N + p.out_cols - 1) / p.out_cols, p.row_groups);
    return EAVQA_OK;
}

// ------------------------------------------------------------------------------------------------------------------- decode attention
// (lanes per key, waves per head, loads in flight, where V waits: 0 late registers, 1 LDS image, 2 registers)
struct DecodePlan { int lpk, wph, u, vmode; dim3 grid; int block; int lds; };

// Of a call inside the decode kernel's domain (attention_decode.hip: decode_supported).  path: the bits of include/eavqa_test.h.
// One workgroup per CU and a head's keys within two batches of one or two waves: everything in registers, one HBM round trip (path bit 4:
// keep the round-3 LDS-image kernel for A / B measurements and its parity tests).  Taken where it measured faster
// (profiles/round4_decode_attention.md): one wave per head (<= 80 / 40 keys: 9.5 -> 6.6 us) and two waves x 10 loads (T0-3B cross-attention,
// 150 keys x 64: 16.9 -> 13.9 us).  Two waves x 20 loads (OPT-2.7B, 160 keys x 80) landed its 204 KB per CU no sooner than the LDS-image
// kernel (22.6 against 21.1 us): path bit 5 selects it for measurements only.
// Otherwise 4 waves per head when the grid fits the chip once, fewer for larger batches, and the V image rides in LDS only with 4 waves and
// when the WHOLE request (scores + per-wave scratch + image) fits the 150 KiB the kernel opts into; else the register route (small head dims
// at long Sk: hd = 16, Sk ~ 1024 asked for 152 KiB and failed the launch).
inline DecodePlan decode_plan(int B, int H, int Sk, int hd, int path) {
    DecodePlan p;
    p.grid = dim3(B, (H + 3) / 4);
    const int blocks = B * ((H + 3) / 4);
    p.lpk = hd <= 64 ? 8 : 16;
    const int kpi = 64 / p.lpk;                             // keys per load instruction
    p.u = 10;
    if (blocks <= 256 && Sk <= kpi * 2 * ((path & 32) ? 20 : 10) && !(path & 16)) {
        p.vmode = 2;
        p.wph = Sk <= kpi * 10 ? 1 : 2;
        p.u = Sk <= kpi * p.wph * 10 ? 10 : 20;
        p.lds = (4 * Sk + 4 * p.wph * 128) * (int)sizeof(float);
    } else {
        p.wph = blocks <= 256 ? 4 : (blocks <= 512 ? 2 : 1);
        const int v_image = Sk * 4 * hd * 2, lds_base = (4 * Sk + 4 * p.wph * 128) * (int)sizeof(float);
        p.vmode = p.wph == 4 && lds_base + v_image <= DECODE_LDS_MAX;
        p.lds = lds_base + (p.vmode ? v_image : 0);
    }
    p.block = 256 * p.wph;
    return p;
}

// what the host-only eavqa_*_route entry points write
inline void report(eavqa_launch_plan_t* out, int v0, int v1, int v2, int v3, dim3 grid, int block, int lds) {
    if (!out) return;
    out->variant[0] = v0; out->variant[1] = v1; out->variant[2] = v2; out->variant[3] = v3;
    out->grid_x = (int)grid.x; out->grid_y = (int)grid.y; out->block = block; out->lds_bytes = lds;
}

}  // namespace
