// Decode-step GEMM without partial sums (eavqa_gemm_decode in include/eavqa.h): C[M <= 64, N] = epilogue(norm(A) B^T), B = a frozen
// [N, K] weight read ONCE from HBM.
//
// Why a second decode GEMM beside the split-K one (decode.hip): split-K over workgroups keeps the activation traffic low (a
// workgroup's A slice is staged once for 128 columns) but leaves ks x M x N fp32 partial sums that somebody has to add up - a finish
// pass or a LayerNorm pass per GEMM, i.e. three extra 5-6 us kernels in an eight-kernel layer of 86 us (OPT-2.7B, B = 32).  Here K is
// split over the EIGHT WAVES OF ONE WORKGROUP instead: the workgroup owns 16 NF weight rows (columns of C) and all of K, wave w takes
// the 64-deep k-blocks w, w + 8, ...; its operands go global -> registers -> MFMA with no LDS in between (nothing is shared between
// waves: their k-blocks are disjoint), the eight accumulator sets meet in LDS once, and the epilogue - bias, activation, T5's gate,
// residual, output in up to three column segments (q | K-cache row | V-cache row) - runs on the finished sums.  What that buys:
//   * no partial sums, no finish kernels: a decoder layer is QKV, attention, out-proj, FFN-up, FFN-down = 5 kernels;
//   * LayerNorm / RMSNorm of the A operand is applied WHILE LOADING it (a_kind 1 / 2: A is the fp32 residual stream): the statistics
//     of a row come from the producing GEMM of that stream, which leaves one (sum, M2) pair per row and workgroup (`stats_out`,
//     combined here in a fixed order with Chan's update - bitwise reproducible, no atomics);
//   * a whole 128-byte line per weight row and load instruction pair (the two halves of a 64-deep k-block: each instruction fetches a
//     contiguous 64-byte piece of 16 rows - four lanes side by side; a lane owning 32 consecutive bytes instead makes every
//     instruction gather four separate 16-byte pieces per row and measured 35 GB/s per CU).
// What it costs: every workgroup reads ALL of A (M x K), from L2.  At M = 32 that is as many bytes as its own weights when it owns 32
// columns, twice as many with 16: fine for K = E (A = 160 KB), the reason FFN-down (K = 4 E) is the shape to measure against split-K.
#include "decode_params.h"

namespace {

struct DDArgs {
    const void* A; int64_t lda;               // bf16 [M, K] (a_kind 0) or fp32 [M, K] (a_kind 1 LayerNorm, 2 RMSNorm)
    const float* gamma; const float* beta;    // [K] fp32 (beta NULL for RMSNorm)
    const float2* stats_in; int n_stats_in; int stats_in_cols;     // [M][n_stats_in] (sum, M2) over stats_in_cols columns each
    float eps; int a_kind;
    const bf16_t* B; int64_t ldb;             // [N or 2 gate_rows, K]
    int M, N, K;                              // N = output columns (gated: F)
    int gate_rows;                            // 0, or F: output c = act(row c) * (row F + c)
    const float* bias; int act;
    const float* residual; int64_t ldr;
    int out_f32; int seg_cols; FinishSeg seg[3];
    float2* stats_out;                        // [M][gridDim.x] or NULL
    int nt;                                   // weight loads with the non-temporal hint
    unsigned a_bytes, b_bytes;                // extents of A and B for the buffer descriptors (< 2 GB)
    int rotate;                               // workgroup b starts its walk over K at its b-th block (every workgroup reads the same A)
};

// 16-byte buffer loads: a lane whose k-block lies past the end of K gets a byte offset beyond the descriptor's range - the range check
// returns zeros and makes no memory request - so the K loop has NO branches around its loads (with `if (block < count) load` hipcc
// merged the register ring into one set and waited vmcnt(0) after every block: one block in flight, 25 GB/s per CU).
typedef __attribute__((vector_size(16))) unsigned int u32x4_t;
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr unsigned OOB = DIRECT_OOB;               // buffers are < 2 GB (checked on the host)
template <bool NT> __device__ __forceinline__ bf16x8 ldb16(rsrc_t r, unsigned off) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, NT ? 2 : 0));
}
__device__ __forceinline__ float4 ldf4(rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}

__device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (bf16_t)v[e];
    return r;
}

// Chan's parallel update of (count, mean, M2) with a second group; branch-free (an empty group, nb = 0, changes nothing): a branch per
// partial made hipcc wait vmcnt(0) - for the weight window - at every join
__device__ __forceinline__ void chan(float& n, float& mean, float& m2, float nb, float meanb, float m2b) {
    const float nn = n + nb, d = meanb - mean;
    const float f = nb > 0.f ? nb * fast_rcp(nn) : 0.f;
    mean += d * f;
    m2 += m2b + d * d * n * f;
    n = nn;
}

// MF: 16-row fragments of A (M <= 16 MF); NF: 16-column fragments per workgroup; AF32: A is the fp32 stream, normalised on load.
// U: k-blocks in flight per wave (vmcnt counts in order, so A and B of a block travel together: depth U for both)
template <int MF, int NF, bool AF32> struct DDCfg {
    static constexpr int per_block = 8 * NF + (AF32 ? 16 : 8) * MF;
    static constexpr int budget = AF32 ? 112 : 150;            // registers of the window (the fp32 form also holds the converted operands)
    static constexpr int U = budget / per_block > 8 ? 8 : (budget / per_block < 2 ? 2 : budget / per_block);
};

template <int MF, int NF, bool AF32, bool NT>
__global__ __launch_bounds__(512) void gemm_decode_direct_kernel(const DDArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ROWS = 16 * MF, COLS = 16 * NF, PITCH = COLS + 4, U = DDCfg<MF, NF, AF32>::U;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x = lane & 15, g = lane >> 4;
    const int K = p.K, M = p.M;
    const int nblk = K >> 6;
    const int cnt = (nblk - wave + 7) >> 3;                       // this wave's k-blocks: wave, wave + 8, ...
    const int rot = (p.rotate && cnt > 0) ? (int)(blockIdx.x % (unsigned)cnt) : 0;
    auto blk = [&](int s) { const int t = s + rot; return t >= cnt ? t - cnt : t; };      // s-th block of this wave's walk
    const int out_cols = p.gate_rows ? COLS / 2 : COLS;
    const int n0 = blockIdx.x * out_cols;

    // LDS: [gamma K][beta K][mean ROWS][rstd ROWS] during the K loop (AF32), then the 8 accumulator slabs + one output tile
    float* s_gamma = reinterpret_cast<float*>(smem);
    float* s_beta = s_gamma + K;
    float* s_mean = s_beta + K;
    float* s_rstd = s_mean + 64;
    float* red = reinterpret_cast<float*>(smem);                  // [8][ROWS][PITCH]
    float* tile = red + 8 * ROWS * PITCH;                         // [ROWS][COLS + 1]

    // ---- 1. (AF32) what the A operand waits for goes out first: gamma / beta by LDS-DMA (no registers), then this workgroup's rows'
    //         statistics partials - TPR threads per row, NQ partials each, ALL issued at once through a range-checked descriptor (no
    //         branches: a loop of guarded loads made hipcc wait vmcnt(0) per pass, behind the weight loads below)
    constexpr int TPR = 512 / ROWS, NQ = 256 / TPR;               // n_stats_in <= 256 (checked on the host)
    const int m0 = blockIdx.y * ROWS;
    const int srow = tid / TPR, spart = tid % TPR;
    float2 st[AF32 ? NQ : 1];
    if (AF32) {
        for (int base = wave * 64; base < K / 4; base += 512) {
            const int c = base + lane;
            if (c < K / 4) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.gamma + 4 * c),
                                                 (__attribute__((address_space(3))) void*)(s_gamma + 4 * base), 16, 0, 0);
                if (p.beta)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.beta + 4 * c),
                                                     (__attribute__((address_space(3))) void*)(s_beta + 4 * base), 16, 0, 0);
            }
        }
        const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(p.stats_in), 0, (unsigned)(M * p.n_stats_in * 8), 0x00020000);
        const unsigned row_off = m0 + srow < M ? (unsigned)((m0 + srow) * p.n_stats_in * 8) : OOB;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int i = spart + TPR * q;
            st[q] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, i < p.n_stats_in ? row_off + 8u * i : OOB, 0, 0));
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- 2. weight rows of this lane; the first U blocks of B
    const rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.B), 0, p.b_bytes, 0x00020000);
    const rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, p.a_bytes, 0x00020000);
    unsigned bo[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        int n;
        if (p.gate_rows) {
            const int half = NF / 2, jj = j < half ? j : j - half;
            n = min(n0 + 16 * jj + x, p.N - 1) + (j < half ? 0 : p.gate_rows);
        } else {
            n = min(n0 + 16 * j + x, p.N - 1);
        }
        bo[j] = (unsigned)(((int64_t)n * p.ldb + wave * 64 + 8 * g) * 2);
    }
    bf16x8 wlo[U][NF], whi[U][NF];
    auto load_w = [&](int u, int s) {                 // block s of this wave = k-block wave + 8 s: 512 elements further along the row
        const unsigned step = s < cnt ? (unsigned)blk(s) * 1024u : OOB;
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            wlo[u][j] = ldb16<NT>(rb, bo[j] + step);
            whi[u][j] = ldb16<NT>(rb, bo[j] + step + 64);
        }
    };
    unsigned ao[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
        ao[i] = (unsigned)(((int64_t)min(m0 + 16 * i + x, M - 1) * p.lda + wave * 64 + 8 * g) * (AF32 ? 4 : 2));
    bf16x8 alo[AF32 ? 1 : U][MF], ahi[AF32 ? 1 : U][MF];
    float4 araw[AF32 ? U : 1][MF][4];
    auto load_a = [&](int u, int s) {
        const unsigned step = s < cnt ? (unsigned)blk(s) * (AF32 ? 2048u : 1024u) : OOB;
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            if (AF32) {
#pragma unroll
                for (int c = 0; c < 4; ++c) araw[u][i][c] = ldf4(ra, ao[i] + step + 16 * (c & 1) + 128 * (c >> 1));
            } else {
                alo[u][i] = ldb16<false>(ra, ao[i] + step);
                ahi[u][i] = ldb16<false>(ra, ao[i] + step + 64);
            }
        }
    };
    // (sched_barrier: the window must be ISSUED in slot order - the loop waits for slot 0 first, and the waits at the loop head cover both
    // ways into it; hipcc had turned the prologue round, so every iteration began with vmcnt(0))
    if (!AF32) {
#pragma unroll
        for (int u = 0; u < U; ++u) { load_a(u, u); load_w(u, u); __builtin_amdgcn_sched_barrier(0); }
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u) { load_w(u, u); __builtin_amdgcn_sched_barrier(0); }
    }

    // ---- 3. (AF32) row statistics: a thread folds its partials in index order (Chan), then the TPR lanes of a row pairwise
    float rmean[MF], rrstd[MF];
    if (AF32) {
        float n = 0.f, mean = 0.f, m2 = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int i = spart + TPR * q;
            const float nb = i < p.n_stats_in ? (float)min(p.stats_in_cols, K - i * p.stats_in_cols) : 0.f;
            chan(n, mean, m2, nb, st[q].x * fast_rcp(fmaxf(nb, 1.f)), st[q].y);     // (no branch: see chan)
        }
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) {
            const float nb = __shfl_xor(n, o, 64), mb = __shfl_xor(mean, o, 64), qb = __shfl_xor(m2, o, 64);
            // both partners must end with the same bits: the lower lane of the pair is always the left operand
            const bool lo = (spart & o) == 0;
            float n1 = lo ? n : nb, me1 = lo ? mean : mb, q1 = lo ? m2 : qb;
            chan(n1, me1, q1, lo ? nb : n, lo ? mb : mean, lo ? qb : m2);
            n = n1; mean = me1; m2 = q1;
        }
        if (spart == 0) {
            const float inv = 1.f / (float)K;
            if (p.a_kind == 2) {                                  // RMSNorm: mean(x^2) = (M2 + n mean^2) / n
                s_mean[srow] = 0.f;
                s_rstd[srow] = rsqrtf((m2 + n * mean * mean) * inv + p.eps);
            } else {
                s_mean[srow] = mean;
                s_rstd[srow] = rsqrtf(m2 * inv + p.eps);
            }
        }
        // the LDS-DMA of gamma / beta is older than the statistics loads just consumed; the wait below leaves only the U weight blocks
        // issued after them in flight
        __builtin_amdgcn_s_waitcnt(0x0F70 | ((2 * U * NF) & 0xF) | (((2 * U * NF) >> 4) << 14));
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            rmean[i] = s_mean[16 * i + x];                        // rows past M hold the statistics of nothing: their products are never stored
            rrstd[i] = s_rstd[16 * i + x];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { load_a(u, u); __builtin_amdgcn_sched_barrier(0); }
    }

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- 4. K loop, branch-free inside: slot u is refilled with block s + U right BEHIND the MFMAs that read it (the load overwrites the
    //         registers the MFMAs were issued from: no copies, so no loop-carried register moves that would wait for every load in
    //         flight); blocks past the end load zeros (no memory request) and multiply zeros
    for (int s0 = 0; s0 < cnt; s0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = s0 + u;
            if (AF32) {
                const int kb = min((wave + 8 * blk(min(s, max(cnt - 1, 0)))) * 64, K - 64) + 8 * g;
                float4 gm[4], bt[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    gm[c] = *reinterpret_cast<const float4*>(s_gamma + kb + 4 * (c & 1) + 32 * (c >> 1));
                    bt[c] = p.beta ? *reinterpret_cast<const float4*>(s_beta + kb + 4 * (c & 1) + 32 * (c >> 1)) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                bf16x8 al[MF], ah[MF];
#pragma unroll
                for (int i = 0; i < MF; ++i) {
                    float v[16];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float4 r = araw[u][i][c];
                        v[4 * c + 0] = (r.x - rmean[i]) * rrstd[i] * gm[c].x + bt[c].x;
                        v[4 * c + 1] = (r.y - rmean[i]) * rrstd[i] * gm[c].y + bt[c].y;
                        v[4 * c + 2] = (r.z - rmean[i]) * rrstd[i] * gm[c].z + bt[c].z;
                        v[4 * c + 3] = (r.w - rmean[i]) * rrstd[i] * gm[c].w + bt[c].w;
                    }
                    al[i] = pack8(reinterpret_cast<const float (&)[8]>(v[0]));
                    ah[i] = pack8(reinterpret_cast<const float (&)[8]>(v[8]));
                }
                load_a(u, s + U);
#pragma unroll
                for (int i = 0; i < MF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], wlo[u][j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], whi[u][j], acc[i][j], 0, 0, 0);
                    }
                load_w(u, s + U);
            } else {
#pragma unroll
                for (int i = 0; i < MF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo[u][i], wlo[u][j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi[u][i], whi[u][j], acc[i][j], 0, 0, 0);
                    }
                load_a(u, s + U);
                load_w(u, s + U);
            }
            // nothing crosses a block boundary: left alone, the scheduler hoists every MFMA of the U blocks to the top of the loop body
            // behind one vmcnt(0) - the whole window drained once per iteration
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- 5. the eight accumulator sets meet in LDS (gamma / beta are dead: their space is reused behind a barrier)
    if (AF32) __syncthreads();
    {
        float* slab = red + wave * ROWS * PITCH;
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) slab[(16 * i + 4 * g + r) * PITCH + 16 * j + x] = acc[i][j][r];
    }
    __syncthreads();
    const bool want_stats = p.stats_out != nullptr;
    for (int e = tid; e < ROWS * out_cols; e += 512) {
        const int row = e / out_cols, c = e - row * out_cols;
        const int m = m0 + row, n = n0 + c;
        float v = 0.f, v2 = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {                            // wave order: the sum does not depend on scheduling
            v += red[(w * ROWS + row) * PITCH + c];
            if (p.gate_rows) v2 += red[(w * ROWS + row) * PITCH + out_cols + c];
        }
        const bool ok = m < M && n < p.N;
        if (ok) {
            if (p.bias) { v += p.bias[n]; if (p.gate_rows) v2 += p.bias[p.gate_rows + n]; }
            v = act_fwd(p.act, v);
            if (p.gate_rows) v *= v2;
            if (p.residual) v += p.residual[(int64_t)m * p.ldr + n];
            const int sg = n / p.seg_cols, nl = n - sg * p.seg_cols;
            const FinishSeg d = sg == 0 ? p.seg[0] : (sg == 1 ? p.seg[1] : p.seg[2]);
            if (p.out_f32) reinterpret_cast<float*>(d.dst)[(int64_t)m * d.ld + nl] = v;
            else reinterpret_cast<bf16_t*>(d.dst)[(int64_t)m * d.ld + nl] = (bf16_t)v;
        }
        if (want_stats) tile[row * (COLS + 1) + c] = ok ? v : 0.f;
    }
    if (want_stats) {
        __syncthreads();
        if (tid < ROWS && m0 + tid < M) {
            const int nv = min(out_cols, p.N - n0);
            const float* t = tile + tid * (COLS + 1);
            float s = 0.f;
            for (int c = 0; c < nv; ++c) s += t[c];
            const float mu = s / (float)nv;
            float q = 0.f;
            for (int c = 0; c < nv; ++c) { const float d = t[c] - mu; q += d * d; }
            p.stats_out[(int64_t)(m0 + tid) * gridDim.x + blockIdx.x] = make_float2(s, q);
        }
    }
}

// f(kernel) for the plan's variant: every instantiated direct kernel is named here (decode_params.h: direct_instantiated)
template <typename F> bool with_direct_kernel(const DirectPlan& p, F&& f) {
    return with_value<1, 2, 4>(p.mf, [&](auto MF) {
        return with_value<1, 2, 3, 4>(p.nf, [&](auto NF) {
            return with_value<0, 1>(p.af32, [&](auto AF32) {
                constexpr int mf = decltype(MF)::value, nf = decltype(NF)::value;
                constexpr bool af32 = decltype(AF32)::value != 0;
                if constexpr (direct_instantiated(mf, nf, af32)) {
                    if (p.nt) f(KernelTag<gemm_decode_direct_kernel<mf, nf, af32, true>>{});
                    else f(KernelTag<gemm_decode_direct_kernel<mf, nf, af32, false>>{});
                    return true;
                }
                return false;
            });
        });
    });
}

// the kernel argument of a call; the operands' extents are the last thing a call can fail on
int fill_args(const eavqa_decode_gemm_t& a, const DirectPlan& plan, int sel, DDArgs& p) {
    p = {};
    p.A = a.A; p.lda = a.lda; p.gamma = a.gamma; p.beta = a.beta;
    p.stats_in = reinterpret_cast<const float2*>(a.stats_in); p.n_stats_in = a.n_stats_in; p.stats_in_cols = a.stats_in_cols;
    p.eps = a.eps; p.a_kind = a.a_kind;
    p.B = reinterpret_cast<const bf16_t*>(a.B); p.ldb = a.ldb;
    p.M = a.M; p.N = a.N; p.K = a.K; p.gate_rows = a.gated_rows;
    p.bias = a.bias; p.act = a.act; p.residual = a.residual; p.ldr = a.ld_residual;
    p.out_f32 = a.out_f32; p.seg_cols = a.N / a.n_seg;
    for (int i = 0; i < 3; ++i) { p.seg[i].dst = a.out[i]; p.seg[i].ld = a.ld_out[i]; }
    p.stats_out = reinterpret_cast<float2*>(a.stats_out);
    p.nt = plan.nt;
    if (const int rc = direct_extents(a.M, a.N, a.K, a.lda, a.ldb, plan.af32, a.gated_rows, p.a_bytes, p.b_bytes)) return rc;
    // timing-only ablations (RESULTS ARE WRONG): an empty descriptor drops every load through it while the instruction stream stays
    if (sel & 0x20) p.a_bytes = 0;
    if (sel & 0x40) p.b_bytes = 0;
    p.rotate = (sel & 0x80) ? 1 : 0;
    return EAVQA_OK;
}

// both entry points: validate, plan, opt in, fill args, launch
int gemm_decode(const eavqa_decode_gemm_t* a, hipStream_t stream, int sel) {
    if (!a) return EAVQA_E_ARG;
    if (const int rc = validate(*a)) return rc;
    DirectPlan plan;
    if (const int rc = direct_plan(a->M, a->N, a->K, a->a_kind, a->gated_rows != 0, sel, plan)) return rc;
    int rc = EAVQA_E_SHAPE;                                     // (no such variant: the plan and the dispatcher disagree)
    with_direct_kernel(plan, [&](auto k) {
        constexpr auto kernel = decltype(k)::value;
        if (plan.lds > 48 * 1024 && (rc = opt_in_lds<kernel>(DECODE_LDS_MAX))) return;
        DDArgs p;
        if ((rc = fill_args(*a, plan, sel, p))) return;
        hipLaunchKernelGGL(kernel, plan.grid, dim3(512), plan.lds, stream, p);
        rc = hipGetLastError() != hipSuccess ? EAVQA_E_LAUNCH : EAVQA_OK;
    });
    return rc;
}

}  // namespace

extern "C" int eavqa_gemm_decode(const eavqa_decode_gemm_t* args, void* stream) { return gemm_decode(args, reinterpret_cast<hipStream_t>(stream), 0); }
extern "C" int eavqa_gemm_decode_ex(const eavqa_decode_gemm_t* args, void* stream, int sel) {
    return gemm_decode(args, reinterpret_cast<hipStream_t>(stream), sel);
}

// The plan of a shape, for the tests (include/eavqa_test.h): the checks of validate() that read M, N, K alone, then direct_plan() and the
// operands' extents at lda = ldb = K.  variant = (MF, NF, fp32 A, non-temporal weight loads).
extern "C" int eavqa_gemm_decode_route(int M, int N, int K, int a_kind, int gated, int sel, eavqa_launch_plan_t* out) {
    if (M <= 0 || M > 64 || N <= 0 || K <= 0) return EAVQA_E_ARG;
    if (K % 64) return EAVQA_E_SHAPE;
    if (a_kind < 0 || a_kind > 2) return EAVQA_E_DTYPE;
    if (a_kind && K > 16384) return EAVQA_E_ARG;
    DirectPlan p;
    if (const int rc = direct_plan(M, N, K, a_kind, gated != 0, sel, p)) return rc;
    unsigned a_bytes, b_bytes;
    if (const int rc = direct_extents(M, N, K, K, K, p.af32, gated ? N : 0, a_bytes, b_bytes)) return rc;
    report(out, p.mf, p.nf, p.af32, p.nt, p.grid, 512, p.lds);
    return EAVQA_OK;
}

extern "C" int eavqa_gemm_decode_cols(int M, int N, int K, int a_kind, int gated) {
    if (M <= 0 || M > 64 || N <= 0 || K <= 0 || K % 64) return 0;
    DirectPlan p;
    return direct_plan(M, N, K, a_kind, gated != 0, 0, p) == EAVQA_OK ? p.out_cols : 0;
}
