// HF logits processors on the device (eavqa_logits_process in include/eavqa.h): RepetitionPenaltyLogitsProcessor ->
// NoRepeatNGramLogitsProcessor -> NoBadWordsLogitsProcessor -> MinLengthLogitsProcessor / MinNewTokensLengthLogitsProcessor
// (transformers/generation/logits_process.py, 5.15) for one decoder step, in place on the float32 score rows.
//
// One 1024-thread workgroup per row.  The rules are SPARSE: they touch at most cur_len + n_bad + 1 elements of the row, so without
// `to_logprobs` the row itself is never streamed - the kernel moves ~R * cur_len elements and its time is a launch plus a few dependent
// LDS / L2 round trips.  With `to_logprobs` (beam search: HF runs its processors on log_softmax(logits)) the row is first replaced by
// (x - M) - lse with M, lse from row_max_lse (csrc/row_lse.h, the pass of beam_row_kernel): R * V * 4 bytes read twice and written once,
// 16 bytes per lane (the second read is expected, not measured, to hit the L2: a row is 128 KB).
//
// Phases, separated by workgroup barriers: [dense write] | history -> LDS | penalty (read-modify-write: only the FIRST occurrence of a
// token acts, as HF's gather / scatter applies it once however often the token occurs) | bans (n-gram, bad words, eos: all store -inf,
// so they may race).  Ids outside [0, V) are never written through.
#include "common.h"
#include "row_lse.h"

namespace {

constexpr int LP_MAX_HISTORY = 2048;

template <bool LOGPROBS>
__global__ __launch_bounds__(BR_THREADS) void logits_process_kernel(int V, float* scores, int64_t ld, const int64_t* __restrict__ history,
                                                                    int64_t ld_history, int cur_len, float penalty, int ngram, int64_t eos,
                                                                    int suppress_eos, const int32_t* __restrict__ bad_words,
                                                                    const int32_t* __restrict__ bad_lens, int n_bad, int bad_width) {
    __shared__ int64_t h[LP_MAX_HISTORY];
    __shared__ float s_m[BR_WAVES], s_s[BR_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    float* x = scores + (int64_t)row * ld;
    if constexpr (LOGPROBS) {
        const bool vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15u) == 0);
        float M, lse;
        row_max_lse(x, V, vec, s_m, s_s, M, lse, [](const float*, int) {});
        for (int c0 = tid * 4; c0 < V; c0 += BR_THREADS * 4) {          // the second read of the row
            float v[4];
            load4(x, c0, V, vec, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (v[j] - M) - lse;
            if (vec && c0 + 3 < V) *reinterpret_cast<float4*>(x + c0) = make_float4(v[0], v[1], v[2], v[3]);
            else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < V) x[c0 + j] = v[j];
        }
    }
    for (int j = tid; j < cur_len; j += BR_THREADS) h[j] = history[(int64_t)row * ld_history + j];
    __syncthreads();                                                    // history staged; the dense write is visible to the edits

    if (penalty != 1.f) {
        for (int j = tid; j < cur_len; j += BR_THREADS) {
            const int64_t tok = h[j];
            if (tok < 0 || tok >= V) continue;
            bool first = true;
            for (int i = 0; i < j; ++i) first = first && h[i] != tok;
            if (!first) continue;
            const float s = x[tok];
            x[tok] = s < 0.f ? s * penalty : s / penalty;
        }
        __syncthreads();                                                // a banned token that is also penalised ends as -inf
    }

    if (ngram > 0 && cur_len >= ngram) {
        const int64_t* suffix = h + (cur_len - ngram + 1);              // the last ngram - 1 tokens
        for (int i = tid; i <= cur_len - ngram; i += BR_THREADS) {
            bool match = true;
            for (int q = 0; q < ngram - 1; ++q) match = match && h[i + q] == suffix[q];
            const int64_t tok = h[i + ngram - 1];
            if (match && tok >= 0 && tok < V) x[tok] = -INFINITY;
        }
    }
    for (int w = tid; w < n_bad; w += BR_THREADS) {
        const int L = bad_lens[w];
        if (L < 1 || L > bad_width || (L > 1 && L > cur_len)) continue;     // a one-token word bans at any history, an empty one included
        const int32_t* word = bad_words + (int64_t)w * bad_width;
        bool match = true;
        for (int q = 0; q < L - 1; ++q) match = match && h[cur_len - (L - 1) + q] == (int64_t)word[q];
        const int tok = word[L - 1];
        if (match && tok >= 0 && tok < V) x[tok] = -INFINITY;
    }
    if (tid == 0 && suppress_eos && eos >= 0 && eos < V) x[eos] = -INFINITY;
}

}  // namespace

extern "C" int eavqa_logits_process(int R, int V, float* scores, int64_t ld, int to_logprobs, const int64_t* history, int64_t ld_history,
                                    int cur_len, float repetition_penalty, int no_repeat_ngram_size, int64_t eos_token_id, int suppress_eos,
                                    const int32_t* bad_words, const int32_t* bad_lens, int n_bad, int bad_width, void* stream) {
    if (R <= 0 || V <= 0 || !scores || cur_len < 0 || (cur_len > 0 && !history)) return EAVQA_E_ARG;
    if (to_logprobs != 0 && to_logprobs != 1) return EAVQA_E_ARG;
    if (!(repetition_penalty > 0.f) || !(repetition_penalty <= FLT_MAX)) return EAVQA_E_ARG;      // also a NaN
    if (no_repeat_ngram_size < 0 || n_bad < 0 || (n_bad > 0 && (!bad_words || !bad_lens || bad_width < 1))) return EAVQA_E_ARG;
    if (suppress_eos != 0 && suppress_eos != 1) return EAVQA_E_ARG;
    if (suppress_eos && eos_token_id < 0) return EAVQA_E_ARG;
    if (ld < V || (cur_len > 0 && ld_history < cur_len)) return EAVQA_E_SHAPE;
    if (cur_len > LP_MAX_HISTORY || n_bad > 1024 || bad_width > 16) return EAVQA_E_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (to_logprobs)
        hipLaunchKernelGGL(logits_process_kernel<true>, dim3(R), dim3(BR_THREADS), 0, s, V, scores, ld, history, ld_history, cur_len,
                           repetition_penalty, no_repeat_ngram_size, eos_token_id, suppress_eos, bad_words, bad_lens, n_bad, bad_width);
    else
        hipLaunchKernelGGL(logits_process_kernel<false>, dim3(R), dim3(BR_THREADS), 0, s, V, scores, ld, history, ld_history, cur_len,
                           repetition_penalty, no_repeat_ngram_size, eos_token_id, suppress_eos, bad_words, bad_lens, n_bad, bad_width);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
