// Ensemble decoding (eavqa_ensemble_combine in include/eavqa.h): the next-token scores of n ensemble members - n prompts of the same
// question, rows ordered (question, member) - folded into ONE row of log-scores per question, which the rule and pick kernels
// (eavqa_logits_process, eavqa_trie_constrain, eavqa_greedy_pick, eavqa_sample_pick) then consume as logits.
//
// Two launches, both HBM-bound (a step reads the B * n member rows twice and writes B rows):
//   stats      one 1024-thread workgroup per MEMBER row: row_max_lse (csrc/row_lse.h) -> stats[row] = (M, lse), so that a member's
//              log-probabilities (x - M) - lse are the bits beam.hip and logits_process.hip produce.  B * n workgroups.
//   combine    one 256-thread workgroup per (question, chunk of 1024 columns): a thread owns 4 consecutive columns, loads them from
//              each of the n member rows (n independent 16-byte loads in flight), reads the n row statistics, combines and stores
//              16 bytes.  B * ceil(V / 1024) workgroups: B alone (32 for the few-shot batch) would leave most of the 256 CUs idle, the
//              chunks (32 for T5's vocabulary) cover the device.
// A thread reads and writes its own columns only; columns >= V are neither read nor written.  16-byte accesses where the leading
// dimension and the pointer allow them (judged separately for `logits` and `out`), the scalar path otherwise, as load4.
#include "common.h"
#include "row_lse.h"

namespace {

constexpr int EC_MAX_N = 8;                    // members per question (eavqa.h names the bound)
constexpr int EC_THREADS = 256;
constexpr int EC_COLS = EC_THREADS * 4;        // columns per workgroup of the combine launch

__global__ __launch_bounds__(BR_THREADS) void ensemble_stats_kernel(int V, const float* __restrict__ logits, int64_t ld,
                                                                    float* __restrict__ stats, float* __restrict__ member_lse) {
    __shared__ float s_m[BR_WAVES], s_s[BR_WAVES];
    const int row = blockIdx.x;
    const bool vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15u) == 0);
    float M, lse;
    row_max_lse(logits + (int64_t)row * ld, V, vec, s_m, s_s, M, lse, [](const float*, int) {});
    if (threadIdx.x == 0) {
        stats[2 * row] = M;
        stats[2 * row + 1] = lse;
        if (member_lse) member_lse[row] = M > -INFINITY ? M + lse : -INFINITY;
    }
}

template <bool MIXTURE>
__global__ __launch_bounds__(EC_THREADS) void ensemble_combine_kernel(int n, int V, const float* __restrict__ logits, int64_t ld,
                                                                      const float* __restrict__ weights, const float* __restrict__ stats,
                                                                      float* __restrict__ out, int64_t ld_out) {
    const int q = blockIdx.y;
    const int c0 = (blockIdx.x * EC_THREADS + threadIdx.x) * 4;
    if (c0 >= V) return;
    const bool vin = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15u) == 0);
    const bool vout = (ld_out % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0);

    // lp[i][j]: member i's log-probability of column c0 + j; a member that is not counted (w = 0) is never loaded
    float w[EC_MAX_N], lp[EC_MAX_N][4];
#pragma unroll
    for (int i = 0; i < EC_MAX_N; ++i) {
        w[i] = 0.f;
        if (i < n) w[i] = weights ? weights[i] : 1.f / (float)n;
        if (w[i] > 0.f) {
            const int64_t row = (int64_t)q * n + i;
            const float M = stats[2 * row], lse = stats[2 * row + 1];
            float v[4];
            load4(logits + row * ld, c0, V, vin, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) lp[i][j] = (M > -INFINITY && v[j] > -INFINITY) ? (v[j] - M) - lse : -INFINITY;   // (a row of -inf: no -inf - -inf)
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) lp[i][j] = -INFINITY;
        }
    }

    float r[4];
    if constexpr (!MIXTURE) {
        // sum_i w_i lp_i over the counted members, in member order: a counted -inf gives -inf, an uncounted one is never multiplied
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = 0.f;
#pragma unroll
        for (int i = 0; i < EC_MAX_N; ++i)
            if (w[i] > 0.f)
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] += w[i] * lp[i][j];
    } else {
        // m + log sum_i w_i exp(lp_i - m), m the largest counted lp_i; all of them -inf: -inf, and no exponent is formed
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float m = -INFINITY;
#pragma unroll
            for (int i = 0; i < EC_MAX_N; ++i) m = fmaxf(m, lp[i][j]);          // (uncounted members hold -inf)
            float s = 0.f;
            if (m > -INFINITY) {
#pragma unroll
                for (int i = 0; i < EC_MAX_N; ++i)
                    if (w[i] > 0.f) s += w[i] * expf(lp[i][j] - m);
            }
            r[j] = m > -INFINITY ? m + logf(s) : -INFINITY;
        }
    }

    float* o = out + (int64_t)q * ld_out;
    if (vout && c0 + 3 < V) *reinterpret_cast<float4*>(o + c0) = make_float4(r[0], r[1], r[2], r[3]);
    else
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < V) o[c0 + j] = r[j];
}

}  // namespace

extern "C" int eavqa_ensemble_combine(int B, int n, int V, const float* logits, int64_t ld, int mode, const float* weights, float* out,
                                      int64_t ld_out, float* stats, float* member_lse, void* stream) {
    if (!logits || !out || !stats) return EAVQA_E_ARG;
    if (B <= 0 || V <= 0 || n < 1 || n > EC_MAX_N) return EAVQA_E_ARG;
    if (mode != EAVQA_ENSEMBLE_PRODUCT && mode != EAVQA_ENSEMBLE_MIXTURE) return EAVQA_E_ARG;
    if (ld < V || ld_out < V) return EAVQA_E_ARG;
    if (static_cast<const void*>(out) == static_cast<const void*>(logits)) return EAVQA_E_ARG;
    if (B > 65535 || (int64_t)B * n > (int64_t)INT32_MAX / 2) return EAVQA_E_SHAPE;          // grid.y; the stats index
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ensemble_stats_kernel, dim3(B * n), dim3(BR_THREADS), 0, s, V, logits, ld, stats, member_lse);
    EAVQA_LAUNCH_CHECK();
    const dim3 grid((V + EC_COLS - 1) / EC_COLS, B);
    if (mode == EAVQA_ENSEMBLE_MIXTURE)
        hipLaunchKernelGGL(ensemble_combine_kernel<true>, grid, dim3(EC_THREADS), 0, s, n, V, logits, ld, weights, stats, out, ld_out);
    else
        hipLaunchKernelGGL(ensemble_combine_kernel<false>, grid, dim3(EC_THREADS), 0, s, n, V, logits, ld, weights, stats, out, ld_out);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
