// Answer-candidate scoring (eavqa_token_logprobs, eavqa_candidate_rank, eavqa_attention_merge in include/eavqa.h): the log-probability
// of given tokens under given logit rows, the per-candidate sums with their ranking, and the merge of two attention segments by their
// log-sum-exp (a prompt shared by several continuations: one segment over the prompt's keys, one over the continuation's own).
//
// token_logprobs: one 1024-thread workgroup per row.  The row is streamed ONCE (row_max_lse of csrc/row_lse.h, the pass of
//   logits_process_kernel: (x - M) - lse is then the same bits as eavqa_logits_process(to_logprobs = 1) stores), after which up to 64
//   threads gather one label each.  R * V * 4 bytes read, R * n_labels * 4 written.
// candidate_rank: one 1024-thread workgroup per question, thread c owns candidate c: a T-term sum in index order, then its rank by
//   counting the candidates that come before it (C <= 1024 comparisons against LDS).  A few KiB in all: the time is the launch.
// attention_merge: elementwise, one thread per 4 output columns (a head is a multiple of 4 columns, so a thread sees one head's pair of
//   weights); B C T H hd elements read twice and written once.
#include "common.h"
#include "row_lse.h"

namespace {

constexpr int TL_MAX_LABELS = 64;
constexpr int CR_MAX_CANDIDATES = 1024;
constexpr int CR_MAX_IGNORED = 16;

__global__ __launch_bounds__(BR_THREADS) void token_logprobs_kernel(int V, const float* __restrict__ logits, int64_t ld,
                                                                    const int64_t* __restrict__ labels, int64_t ld_labels, int n_labels,
                                                                    float* __restrict__ out, int64_t ld_out) {
    __shared__ float s_m[BR_WAVES], s_s[BR_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (int64_t)row * ld;
    const bool vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15u) == 0);
    float M, lse;
    row_max_lse(x, V, vec, s_m, s_s, M, lse, [](const float*, int) {});
    if (tid < n_labels) {
        const int64_t lab = labels[(int64_t)row * ld_labels + tid];
        out[(int64_t)row * ld_out + tid] = (lab >= 0 && lab < V) ? (x[lab] - M) - lse : 0.f;
    }
}

struct IgnoredIds { int64_t id[CR_MAX_IGNORED]; };

// order class of a score: 0 = a number (+inf included), 1 = -inf, 2 = NaN
__device__ __forceinline__ int rank_class(float s) { return s != s ? 2 : (s == -INFINITY ? 1 : 0); }

__global__ __launch_bounds__(CR_MAX_CANDIDATES) void candidate_rank_kernel(int C, int T, float* __restrict__ tok_logp,
                                                                            const int64_t* __restrict__ labels,
                                                                            const int64_t* __restrict__ ignored_ids, int n_ignored,
                                                                            float length_penalty, float* __restrict__ scores,
                                                                            int32_t* __restrict__ n_tokens, int32_t* __restrict__ order) {
    __shared__ float s_score[CR_MAX_CANDIDATES];
    __shared__ int64_t s_ign[CR_MAX_IGNORED];
    const int b = blockIdx.x, c = threadIdx.x;
    if (c < n_ignored) s_ign[c] = ignored_ids[c];
    __syncthreads();
    float score = 0.f;
    if (c < C) {
        const int64_t base = ((int64_t)b * C + c) * T;
        float sum = 0.f;
        int n = 0;
        for (int t = 0; t < T; ++t) {
            const int64_t lab = labels[base + t];
            bool scored = lab >= 0;
            for (int i = 0; i < n_ignored; ++i) scored = scored && lab != s_ign[i];
            if (scored) { sum += tok_logp[base + t]; ++n; }
            else tok_logp[base + t] = 0.f;
        }
        // the exponents a caller normally uses divide without powf (whose last bit is the library's own): 0 = the sum, 1 = the mean
        if (n == 0) score = -INFINITY;
        else if (length_penalty == 0.f) score = sum;
        else if (length_penalty == 1.f) score = sum / (float)n;
        else if (length_penalty == 0.5f) score = sum / sqrtf((float)n);
        else score = sum / powf((float)n, length_penalty);
        scores[(int64_t)b * C + c] = score;
        n_tokens[(int64_t)b * C + c] = n;
        s_score[c] = score;
    }
    __syncthreads();
    if (c < C) {
        const int mine = rank_class(score);
        int before = 0;
        for (int j = 0; j < C; ++j) {
            const float o = s_score[j];
            const int cls = rank_class(o);
            const bool same = cls == mine && (cls != 0 || o == score);
            before += (cls < mine) || (cls == mine && cls == 0 && o > score) || (same && j < c);
        }
        order[(int64_t)b * C + before] = c;
    }
}

// the LSE a segment without a visible key reports: the forward kernels keep masked scores at -FLT_MAX, so the row's maximum stays there
// (m + log(l) = -FLT_MAX, or -FLT_MAX ln 2 where the maximum is kept in base 2); no real score comes near
__device__ __forceinline__ bool lse_empty(float l) { return l < -0.25f * FLT_MAX; }

template <typename T>
__global__ __launch_bounds__(256) void attention_merge_kernel(int64_t n_vec, int C, int Tq, int H, int hd, const T* __restrict__ o1, int64_t ld1,
                                                              const float* __restrict__ lse1, const T* o2, int64_t ld2,
                                                              const float* __restrict__ lse2, T* out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_vec) return;
    const int vec_per_row = H * hd / 4;
    const int64_t row = i / vec_per_row;                 // (b * C + c) * Tq + t
    const int col = (int)(i - row * vec_per_row) * 4;
    const int h = col / hd;
    const int t = (int)(row % Tq);
    const int64_t bc = row / Tq;
    const int64_t b = bc / C;
    const int c = (int)(bc - b * C);
    const float l1 = lse1[(b * H + h) * ((int64_t)C * Tq) + (int64_t)c * Tq + t];
    const float l2 = lse2[(bc * H + h) * Tq + t];
    const float4 a = elem<T>::ld4(o1 + row * ld1 + col);
    const float4 v = elem<T>::ld4(o2 + row * ld2 + col);
    float4 r;
    if (lse_empty(l1)) r = v;                            // (both empty: the second segment's row)
    else if (lse_empty(l2)) r = a;
    else {
        const float m = fmaxf(l1, l2);
        const float w1 = expf(l1 - m), w2 = expf(l2 - m);
        const float inv = 1.f / (w1 + w2);
        r = make_float4((w1 * a.x + w2 * v.x) * inv, (w1 * a.y + w2 * v.y) * inv, (w1 * a.z + w2 * v.z) * inv, (w1 * a.w + w2 * v.w) * inv);
    }
    elem<T>::st4(out + row * ldo + col, r);
}

}  // namespace

extern "C" int eavqa_token_logprobs(int R, int V, const float* logits, int64_t ld, const int64_t* labels, int64_t ld_labels, int n_labels,
                                    float* out, int64_t ld_out, void* stream) {
    if (R <= 0 || V <= 0 || n_labels <= 0 || !logits || !labels || !out) return EAVQA_E_ARG;
    if (ld < V || ld_labels < n_labels || ld_out < n_labels || n_labels > TL_MAX_LABELS) return EAVQA_E_SHAPE;
    hipLaunchKernelGGL(token_logprobs_kernel, dim3(R), dim3(BR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), V, logits, ld, labels,
                       ld_labels, n_labels, out, ld_out);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_candidate_rank(int B, int C, int T, float* tok_logp, const int64_t* labels, const int64_t* ignored_ids, int n_ignored,
                                    float length_penalty, float* scores, int32_t* n_tokens, int32_t* order, void* stream) {
    if (B <= 0 || C <= 0 || T <= 0 || !tok_logp || !labels || !scores || !n_tokens || !order) return EAVQA_E_ARG;
    if (n_ignored < 0 || (n_ignored > 0 && !ignored_ids) || !(length_penalty == length_penalty)) return EAVQA_E_ARG;
    if (C > CR_MAX_CANDIDATES || n_ignored > CR_MAX_IGNORED) return EAVQA_E_SHAPE;
    hipLaunchKernelGGL(candidate_rank_kernel, dim3(B), dim3(CR_MAX_CANDIDATES), 0, reinterpret_cast<hipStream_t>(stream), C, T, tok_logp,
                       labels, ignored_ids, n_ignored, length_penalty, scores, n_tokens, order);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_attention_merge(int dtype, int B, int C, int T, int H, int hd, const void* o1, int64_t ld1, const float* lse1,
                                     const void* o2, int64_t ld2, const float* lse2, void* out, int64_t ldo, void* stream) {
    if (dtype != EAVQA_F32 && dtype != EAVQA_BF16) return EAVQA_E_ARG;
    if (B <= 0 || C <= 0 || T <= 0 || H <= 0 || hd <= 0 || !o1 || !lse1 || !o2 || !lse2 || !out) return EAVQA_E_ARG;
    const int q = dtype == EAVQA_F32 ? 4 : 8;            // a 16-byte piece never crosses a head; rows start on 16 bytes
    const int64_t width = (int64_t)H * hd;
    if (hd % q || ld1 < width || ld2 < width || ldo < width || ld1 % q || ld2 % q || ldo % q) return EAVQA_E_SHAPE;
    if (width > INT32_MAX) return EAVQA_E_SHAPE;
    if (!eavqa_aligned16(o1) || !eavqa_aligned16(o2) || !eavqa_aligned16(out)) return EAVQA_E_ALIGN;
    const int64_t n_vec = (int64_t)B * C * T * (width / 4);
    const int64_t blocks = (n_vec + 255) / 256;
    if (blocks > INT32_MAX) return EAVQA_E_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_F32)
        hipLaunchKernelGGL(attention_merge_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, n_vec, C, T, H, hd,
                           static_cast<const float*>(o1), ld1, lse1, static_cast<const float*>(o2), ld2, lse2, static_cast<float*>(out), ldo);
    else
        hipLaunchKernelGGL(attention_merge_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, n_vec, C, T, H, hd,
                           static_cast<const bf16_t*>(o1), ld1, lse1, static_cast<const bf16_t*>(o2), ld2, lse2, static_cast<bf16_t*>(out), ldo);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
