// Beam search on the device (eavqa_beam_step / eavqa_beam_reorder in include/eavqa.h): one step of HF's GenerationMixin._beam_search
// (transformers/generation/utils.py, 5.15) without a host round trip.
//   beam_row_kernel     one workgroup per decoder row: ONE pass over the row's logits (online max / sum of exponentials and the thread's
//                       best element), then 2k selection rounds - a block arg-max over the threads' current bests, after which only the
//                       thread that owned the winner looks at its own ~V / 1024 elements again (they are still in the L2).  The row is
//                       read from HBM once; the candidates leave as accumulated log-probabilities.
//   beam_merge_kernel   one workgroup per batch item: k-way merge of the rows' sorted lists to the item's top 2k, then the bookkeeping of
//                       HF's steps d - g (next running beams, pool of finished hypotheses, stop heuristic) by one thread, the sequence
//                       gathers by all of them (one thread per position, so the gather is in place).  The last workgroup to finish
//                       writes the step's "continue" flag.
//   beam_reorder_kernel K / V caches gathered by beam parent, 16 bytes per lane, ping -> pong.
#include "common.h"
#include "row_lse.h"

namespace {

constexpr int BEAM_MAX = 8;
constexpr float BEAM_NEG = -1.0e9f;              // HF's sentinel for "cannot be chosen"

// (value, index) order of a descending sort with the smaller index first among equals
__device__ __forceinline__ bool before(float v, int i, float v2, int i2) { return v > v2 || (v == v2 && i < i2); }

// a NaN ranks (and on the log-probability entry leaves) as -inf, as in the sampling pick (warp_temp in sample.hip): before() is false on it from both sides, so a row
// with fewer than 2k other entries would otherwise run out of winners and emit the "none" index 0x7fffffff as a token
__device__ __forceinline__ float rank_of(float v) { return v != v ? -INFINITY : v; }

// LOGPROBS (eavqa_beam_step_logprobs): the row already holds (processed) log-probabilities - no max / log-sum-exp pass, the values rank
// as given (-inf entries last) and leave as value + run_scores[row]
template <bool LOGPROBS>
__global__ __launch_bounds__(BR_THREADS) void beam_row_kernel(int k, int V, const float* __restrict__ logits, int64_t ld,
                                                              const float* __restrict__ run_scores, float* __restrict__ cand_val,
                                                              int32_t* __restrict__ cand_tok) {
    __shared__ float s_m[BR_WAVES], s_s[BR_WAVES], s_v[BR_WAVES];
    __shared__ int s_i[BR_WAVES];
    __shared__ float win_v;
    __shared__ int win_i;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (int64_t)row * ld;
    const bool vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15u) == 0);
    // the one pass: row max / log-sum-exp (row_max_lse) and the thread's best element
    float bv = -INFINITY, M = 0.f, lse = 0.f;
    int bi = 0x7fffffff;
    auto best = [&](const float* v, int c0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = rank_of(v[j]);
            if (c0 + j < V && before(u, c0 + j, bv, bi)) { bv = u; bi = c0 + j; }
        }
    };
    if constexpr (LOGPROBS) {
        for (int c0 = tid * 4; c0 < V; c0 += BR_THREADS * 4) {
            float v[4];
            load4(x, c0, V, vec, v);
            best(v, c0);
        }
    } else {
        row_max_lse(x, V, vec, s_m, s_s, M, lse, best);
    }
    const float acc = run_scores[row];
    for (int r = 0; r < 2 * k; ++r) {
        float v = bv;
        int i = bi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(v, o, 64);
            const int i2 = __shfl_xor(i, o, 64);
            if (before(v2, i2, v, i)) { v = v2; i = i2; }
        }
        if (lane == 0) { s_v[wave] = v; s_i[wave] = i; }
        __syncthreads();
        if (tid == 0) {
            float fv = s_v[0];
            int fi = s_i[0];
            for (int w = 1; w < BR_WAVES; ++w)
                if (before(s_v[w], s_i[w], fv, fi)) { fv = s_v[w]; fi = s_i[w]; }
            win_v = fv; win_i = fi;
            // log_softmax in float32 as torch computes it, plus the beam's running score (HF step b)
            cand_val[(int64_t)row * 2 * k + r] = LOGPROBS ? fv + acc : ((fv - M) - lse) + acc;
            cand_tok[(int64_t)row * 2 * k + r] = fi;
        }
        __syncthreads();
        const float lv = win_v;
        const int li = win_i;
        if (li != 0x7fffffff && ((li >> 2) & (BR_THREADS - 1)) == tid) {      // the owner finds its next element after (lv, li)
            bv = -INFINITY; bi = 0x7fffffff;
            auto next = [&](float u, int c) {
                const float w = rank_of(u);
                if (before(lv, li, w, c) && before(w, c, bv, bi)) { bv = w; bi = c; }
            };
            for (int c0 = tid * 4; c0 < V; c0 += BR_THREADS * 4) {      // (the other threads wait for this one: only the row's last
                float u[4];                                              // group of 4 pays for the bounds checks)
                load4(x, c0, V, vec, u);
                if (c0 + 3 < V) {
                    next(u[0], c0); next(u[1], c0 + 1); next(u[2], c0 + 2); next(u[3], c0 + 3);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j < V) next(u[j], c0 + j);
                }
            }
        }
    }
}

constexpr int BM_THREADS = 256;

__global__ __launch_bounds__(BM_THREADS) void beam_merge_kernel(int B, int k, int cur_len, int max_length, int64_t eos, float pool_div,
                                                                float heur_div, int es_true, const float* __restrict__ cand_val,
                                                                const int32_t* __restrict__ cand_tok, int64_t* next_tokens, int32_t* parents,
                                                                float* run_scores, int64_t* run_seq, int64_t* pool_seq, float* pool_scores,
                                                                int32_t* pool_len, int32_t* pool_fin, int32_t* improve, int32_t* cont,
                                                                int32_t* sync) {
    __shared__ int n_par[BEAM_MAX], n_tok[BEAM_MAX];          // next running beams: parent beam, token
    __shared__ int p_src[BEAM_MAX];                            // new pool slot: old slot (< k) or k + candidate rank
    __shared__ int c_par[2 * BEAM_MAX], c_tok[2 * BEAM_MAX];   // the item's top 2k
    const int b = blockIdx.x, K2 = 2 * k;
    if (threadIdx.x == 0) {
        const float* cv = cand_val + (int64_t)b * k * K2;
        const int32_t* ct = cand_tok + (int64_t)b * k * K2;
        float val[2 * BEAM_MAX];
        bool hit[2 * BEAM_MAX];
        int head[BEAM_MAX];
        for (int i = 0; i < k; ++i) head[i] = 0;
        // top 2k of the k * V candidates: every row's list is sorted, ties go to the smaller flat index beam * V + token
        for (int r = 0; r < K2; ++r) {
            int best = -1;
            float bvv = 0.f;
            int bt = 0;
            for (int i = 0; i < k; ++i) {
                if (head[i] >= K2) continue;
                const float v = cv[i * K2 + head[i]];
                const int t = ct[i * K2 + head[i]];
                if (best < 0 || v > bvv) { best = i; bvv = v; bt = t; }        // equal values: the earlier beam stays
            }
            ++head[best];
            val[r] = bvv; c_par[r] = best; c_tok[r] = bt;
            hit[r] = (int64_t)bt == eos || cur_len + 1 == max_length;
        }
        // e. next running beams (HF: + -1e9 on the hitters, top-k, the earlier rank among equals).  Both the candidates that did not hit
        // and the hitters are in descending order, so this merges the two lists: above -1e9 the first k that did not hit, then the
        // hitters; a candidate at -inf (a token the processors ruled out) ranks below a hitter
        float nscore[BEAM_MAX];
        uint32_t left_hit = 0;
        for (int r = 0; r < K2; ++r) left_hit |= (hit[r] ? 1u : 0u) << r;
        uint32_t left_run = ~left_hit & ((1u << K2) - 1u);
        for (int n = 0; n < k; ++n) {
            const int ra = left_run ? __ffs(left_run) - 1 : K2, rb = left_hit ? __ffs(left_hit) - 1 : K2;
            const float va = ra < K2 ? val[ra] : 0.f, vb = rb < K2 ? val[rb] + BEAM_NEG : 0.f;
            const bool run = rb >= K2 || (ra < K2 && (va > vb || (va == vb && ra < rb)));
            const int r = run ? ra : rb;
            if (run) left_run &= left_run - 1u; else left_hit &= left_hit - 1u;
            n_par[n] = c_par[r]; n_tok[n] = c_tok[r]; nscore[n] = run ? va : vb;
        }
        // f. pool of finished hypotheses: old pool || candidates, top k (stable: the earlier entry wins among equals)
        float old_s[BEAM_MAX], ms[3 * BEAM_MAX];
        int old_l[BEAM_MAX], old_f[BEAM_MAX];
        bool full = true;
        for (int j = 0; j < k; ++j) {
            old_s[j] = pool_scores[b * k + j]; old_l[j] = pool_len[b * k + j]; old_f[j] = pool_fin[b * k + j];
            full = full && old_f[j];
            ms[j] = old_s[j];
        }
        const int imp = improve[b];
        for (int r = 0; r < K2; ++r) {
            float sc = val[r] / pool_div;
            sc += (full && es_true) ? BEAM_NEG : 0.f;
            sc += imp ? 0.f : BEAM_NEG;
            sc += (hit[r] && r < k) ? 0.f : BEAM_NEG;
            ms[k + r] = sc;
        }
        bool taken[3 * BEAM_MAX];
        for (int e = 0; e < k + K2; ++e) taken[e] = false;
        float new_s[BEAM_MAX];
        int new_l[BEAM_MAX], new_f[BEAM_MAX];
        for (int j = 0; j < k; ++j) {
            int best = -1;
            for (int e = 0; e < k + K2; ++e)
                if (!taken[e] && (best < 0 || ms[e] > ms[best])) best = e;
            taken[best] = true;
            p_src[j] = best;
            new_s[j] = ms[best];
            if (best < k) { new_l[j] = old_l[best]; new_f[j] = old_f[best]; }
            else { new_l[j] = cur_len + 1; new_f[j] = (hit[best - k] && best - k < k) ? 1 : 0; }
        }
        bool all_fin = true;
        float worst = new_s[0];
        for (int j = 0; j < k; ++j) {
            pool_scores[b * k + j] = new_s[j]; pool_len[b * k + j] = new_l[j]; pool_fin[b * k + j] = new_f[j];
            all_fin = all_fin && new_f[j];
            worst = fminf(worst, new_s[j]);
        }
        for (int i = 0; i < k; ++i) {
            run_scores[b * k + i] = nscore[i];
            next_tokens[b * k + i] = n_tok[i];
            parents[b * k + i] = b * k + n_par[i];
        }
        // g. _check_early_stop_heuristic after the length increment, and this item's part of the loop condition
        const float best_run = nscore[0] / heur_div;
        bool can = false;
        for (int j = 0; j < k; ++j) can = can || best_run > (new_f[j] ? worst : BEAM_NEG);
        const int imp2 = (imp && can) ? 1 : 0;
        improve[b] = imp2;
        // bit 0: some item can improve; bit 1: some pool slot is open (or early_stopping is not True); bit 2: some candidate did not hit
        int bits = imp2 | ((!all_fin || !es_true) ? 2 : 0);
        for (int r = 0; r < K2; ++r)
            if (!hit[r]) bits |= 4;
        atomicOr(&sync[0], bits);
        __threadfence();
        if (atomicAdd(&sync[1], 1) == B - 1) {               // the last item: publish the flag, leave the words zeroed for the next step
            __threadfence();
            *cont = atomicOr(&sync[0], 0) == 7 ? 1 : 0;
            atomicExch(&sync[0], 0);
            atomicExch(&sync[1], 0);
        }
    }
    __syncthreads();
    // sequences: one thread per position, so every gather reads all of its sources before it writes (in place)
    for (int p = threadIdx.x; p < max_length; p += BM_THREADS) {
        int64_t run[BEAM_MAX], pool[BEAM_MAX];
#pragma unroll
        for (int i = 0; i < BEAM_MAX; ++i)
            if (i < k) {
                run[i] = run_seq[((int64_t)b * k + i) * max_length + p];
                pool[i] = pool_seq[((int64_t)b * k + i) * max_length + p];
            }
        for (int i = 0; i < k; ++i) {
            int64_t v = 0;
#pragma unroll
            for (int q = 0; q < BEAM_MAX; ++q)
                if (q == n_par[i]) v = run[q];
            run_seq[((int64_t)b * k + i) * max_length + p] = p == cur_len ? (int64_t)n_tok[i] : v;
        }
        for (int j = 0; j < k; ++j) {
            const int src = p_src[j];
            int64_t v = 0;
            if (src < k) {
#pragma unroll
                for (int q = 0; q < BEAM_MAX; ++q)
                    if (q == src) v = pool[q];
            } else {
                const int par = c_par[src - k];
#pragma unroll
                for (int q = 0; q < BEAM_MAX; ++q)
                    if (q == par) v = run[q];
                if (p == cur_len) v = c_tok[src - k];
            }
            pool_seq[((int64_t)b * k + j) * max_length + p] = v;
        }
    }
}

// dst[plane][r][j][:] = src[plane][parent[r]][j][:] for j < t; one workgroup per (row r, position j, plane), 16 bytes per lane
__global__ __launch_bounds__(256) void beam_reorder_kernel(int rows, int t, int t_max, int row_vec16, const uint4* __restrict__ src,
                                                           uint4* __restrict__ dst, int64_t plane_vec16,
                                                           const int32_t* __restrict__ parents) {
    const int r = blockIdx.x / t, j = blockIdx.x % t;
    const int par = parents[r];
    if (par < 0 || par >= rows) return;                        // (never by construction: parents come from eavqa_beam_step)
    const uint4* s = src + (int64_t)blockIdx.y * plane_vec16 + ((int64_t)par * t_max + j) * row_vec16;
    uint4* d = dst + (int64_t)blockIdx.y * plane_vec16 + ((int64_t)r * t_max + j) * row_vec16;
    for (int c = threadIdx.x; c < row_vec16; c += 256) d[c] = s[c];
}

}  // namespace

extern "C" int64_t eavqa_beam_step_workspace_bytes(int B, int k) {
    if (B <= 0 || k < 1 || k > BEAM_MAX) return 0;
    return (int64_t)B * k * 2 * k * 8 + 16;                    // candidates (float32 value + int32 token) and the two words of the step's tail
}

static int beam_step(bool logprobs, int B, int k, int V, const float* logits, int64_t ld, int cur_len, int max_length, int64_t eos_token_id,
                     float pool_div, float heur_div, int early_stopping, int64_t* next_tokens, int32_t* parents, float* run_scores,
                     int64_t* run_seq, int64_t* pool_seq, float* pool_scores, int32_t* pool_len, int32_t* pool_fin, int32_t* improve,
                     int32_t* cont, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!logits || !next_tokens || !parents || !run_scores || !run_seq || !pool_seq || !pool_scores || !pool_len || !pool_fin || !improve ||
        !cont || !workspace)
        return EAVQA_E_ARG;
    if (B <= 0 || V <= 0 || cur_len < 1 || cur_len >= max_length) return EAVQA_E_ARG;
    if (k < 1 || k > BEAM_MAX || V < 2 * k || ld < V) return EAVQA_E_SHAPE;
    if (early_stopping < 0 || early_stopping > 2) return EAVQA_E_ARG;
    if (workspace_bytes < eavqa_beam_step_workspace_bytes(B, k)) return EAVQA_E_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 3u) return EAVQA_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * k * 2 * k;
    float* cand_val = static_cast<float*>(workspace);
    int32_t* cand_tok = reinterpret_cast<int32_t*>(cand_val + n);
    int32_t* sync = cand_tok + n;
    if (logprobs) hipLaunchKernelGGL(beam_row_kernel<true>, dim3(B * k), dim3(BR_THREADS), 0, s, k, V, logits, ld, run_scores, cand_val, cand_tok);
    else hipLaunchKernelGGL(beam_row_kernel<false>, dim3(B * k), dim3(BR_THREADS), 0, s, k, V, logits, ld, run_scores, cand_val, cand_tok);
    EAVQA_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(BM_THREADS), 0, s, B, k, cur_len, max_length, eos_token_id, pool_div, heur_div,
                       early_stopping == 1 ? 1 : 0, cand_val, cand_tok, next_tokens, parents, run_scores, run_seq, pool_seq, pool_scores,
                       pool_len, pool_fin, improve, cont, sync);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_beam_step(int B, int k, int V, const float* logits, int64_t ld, int cur_len, int max_length, int64_t eos_token_id,
                               float pool_div, float heur_div, int early_stopping, int64_t* next_tokens, int32_t* parents,
                               float* run_scores, int64_t* run_seq, int64_t* pool_seq, float* pool_scores, int32_t* pool_len,
                               int32_t* pool_fin, int32_t* improve, int32_t* cont, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    return beam_step(false, B, k, V, logits, ld, cur_len, max_length, eos_token_id, pool_div, heur_div, early_stopping, next_tokens, parents,
                     run_scores, run_seq, pool_seq, pool_scores, pool_len, pool_fin, improve, cont, workspace, workspace_bytes, stream);
}

extern "C" int eavqa_beam_step_logprobs(int B, int k, int V, const float* logits, int64_t ld, int cur_len, int max_length,
                                        int64_t eos_token_id, float pool_div, float heur_div, int early_stopping, int64_t* next_tokens,
                                        int32_t* parents, float* run_scores, int64_t* run_seq, int64_t* pool_seq, float* pool_scores,
                                        int32_t* pool_len, int32_t* pool_fin, int32_t* improve, int32_t* cont, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    return beam_step(true, B, k, V, logits, ld, cur_len, max_length, eos_token_id, pool_div, heur_div, early_stopping, next_tokens, parents,
                     run_scores, run_seq, pool_seq, pool_scores, pool_len, pool_fin, improve, cont, workspace, workspace_bytes, stream);
}

extern "C" int eavqa_beam_reorder(int dtype, int n_planes, int rows, int t, int t_max, int inner, const void* src, void* dst,
                                  int64_t plane_stride, const int32_t* parents, void* stream) {
    if (!src || !dst || !parents || src == dst) return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (n_planes <= 0 || rows <= 0 || t <= 0 || t > t_max || inner <= 0 || plane_stride < (int64_t)rows * t_max * inner) return EAVQA_E_ARG;
    const int64_t es = dtype == EAVQA_BF16 ? 2 : 4;
    if ((inner * es) % 16 || (plane_stride * es) % 16 || !eavqa_aligned16(src) || !eavqa_aligned16(dst)) return EAVQA_E_ALIGN;
    if ((int64_t)rows * t > 0x7fffffff || n_planes > 65535) return EAVQA_E_SHAPE;
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(rows * t, n_planes), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rows, t, t_max,
                       (int)(inner * es / 16), static_cast<const uint4*>(src), static_cast<uint4*>(dst), plane_stride * es / 16, parents);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
