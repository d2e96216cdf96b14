// Row maximum and log-sum-exp of one float32 row by one 1024-thread workgroup: the pass beam_row_kernel (csrc/beam.hip) and
// logits_process_kernel (csrc/logits_process.hip) share, so that log-probabilities computed by either are the same bits.
#pragma once
#include "common.h"

namespace {

constexpr int BR_THREADS = 1024;
constexpr int BR_WAVES = BR_THREADS / EAVQA_WAVE;

// the 4 columns c0 .. c0 + 3 of a row; columns >= V are never read (the head leaves its pad columns unwritten)
__device__ __forceinline__ void load4(const float* x, int c0, int V, bool vec, float* v) {
    if (vec && c0 + 3 < V) {
        const float4 t = *reinterpret_cast<const float4*>(x + c0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c0 + j < V ? x[c0 + j] : -INFINITY;
    }
}

// ONE pass over x[0 : V]: online max / sum of exponentials per thread (4 columns at a time, stride 4 * BR_THREADS), then the row's
// M = max and lse = log(sum exp(x - M)) in a fixed order (lanes by xor tree, waves in index order).  log_softmax is (x - M) - lse.
// `visit(v, c0)` sees every group of 4 loaded values (for the caller's own per-thread bookkeeping).  s_m / s_s: BR_WAVES floats of LDS
// each.  Every thread of the workgroup has to call it (two barriers).
template <typename Visit>
__device__ __forceinline__ void row_max_lse(const float* x, int V, bool vec, float* s_m, float* s_s, float& M_out, float& lse_out, Visit visit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = -INFINITY, s = 0.f;
    for (int c0 = tid * 4; c0 < V; c0 += BR_THREADS * 4) {
        float v[4];
        load4(x, c0, V, vec, v);
        const float m4 = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        if (m4 > m) { s *= expf(m - m4); m = m4; }
        if (m > -INFINITY) s += expf(v[0] - m) + expf(v[1] - m) + expf(v[2] - m) + expf(v[3] - m);
        visit(v, c0);
    }
    const float wm = wave_max(m);
    if (lane == 0) s_m[wave] = wm;
    __syncthreads();
    float M = s_m[0];
#pragma unroll
    for (int w = 1; w < BR_WAVES; ++w) M = fmaxf(M, s_m[w]);
    const float ws = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    if (lane == 0) s_s[wave] = ws;
    __syncthreads();
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < BR_WAVES; ++w) S += s_s[w];
    M_out = M;
    lse_out = logf(S);
}

}  // namespace
