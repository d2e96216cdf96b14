// RICES retrieval on the GPU: brute-force inner-product k-nearest-neighbours over
// L2-normalised CLIP text embeddings, the arithmetic of src/in_context_example_selection/get_question_knn.py:64-76
// (faiss.normalize_L2 + IndexFlatIP.search, k = 2048 over ~443 k x 768).  The scores are one exact-fp32 eavqa_gemm
// per query tile; this file holds the two HBM-bound pieces around it:
//
//   eavqa_l2_normalize_rows   x[r, :] /= ||x[r, :]||_2   (rows of norm 0 are left alone, as faiss does)
//   eavqa_topk_rows           per row: the k largest scores, sorted descending, ties broken by the smaller column
//   eavqa_rices_joint_scores  joint[i, j] = text_sim[i, j] + <query image i, train image of text neighbour j>  (see below)
//
// Top-k: one 1024-thread workgroup per row.  (1) radix select on the order-preserving integer image of the floats,
// four 8-bit passes with an LDS histogram each, finds the k-th largest key T; (2) every wave owns a contiguous segment
// of the row, counts its elements > T and == T, and after an exclusive scan over the 16 waves writes them at positions
// that depend only on the data (ballot + popcount inside the wave): elements equal to T are kept in column order until
// k is reached; (3) the k (key, column) pairs are bitonic-sorted in LDS.  The row is read six times (it stays in L2
// for rows up to a few MB); nothing depends on scheduling, so the result is bitwise reproducible.
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t key_of(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;                           // -0 compares equal to +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // ascending in the float order (NaNs at the ends)
}
__device__ __forceinline__ float value_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void l2_normalize_kernel(int rows, int cols, float* x, int64_t ld) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    float* p = x + (int64_t)row * ld;
    float s = 0.f;
    for (int c = threadIdx.x; c < cols; c += 256) { const float v = p[c]; s += v * v; }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float nr = (red[0] + red[1]) + (red[2] + red[3]);
    if (nr > 0.f) {
        const float inv = 1.f / sqrtf(nr);
        for (int c = threadIdx.x; c < cols; c += 256) p[c] *= inv;
    }
}

constexpr int TK_THREADS = 1024, TK_WAVES = 16, TK_MAX = 2048;

__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(int cols, const float* __restrict__ scores, int64_t ld, int k,
                                                               float* __restrict__ out_val, int64_t* __restrict__ out_idx) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[2];                       // [0] prefix found so far, [1] how many of the k remain below it
    __shared__ uint32_t wave_gt[TK_WAVES], wave_eq[TK_WAVES];
    __shared__ unsigned long long cand[TK_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = scores + (int64_t)blockIdx.x * ld;

    // ---- (1) k-th largest key by radix select, most significant byte first
    uint32_t prefix = 0, mask = 0, want = (uint32_t)k;   // `want`: rank (1-based, from the top) inside the current bucket
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int c = tid; c < cols; c += TK_THREADS) {
            const uint32_t key = key_of(x[c]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            int b = 255;
            for (; b > 0; --b) {
                if (acc + hist[b] >= want) break;
                acc += hist[b];
            }
            sel[0] = prefix | ((uint32_t)b << shift);
            sel[1] = want - acc;
        }
        __syncthreads();
        prefix = sel[0];
        want = sel[1];
        mask |= 255u << shift;
        __syncthreads();
    }
    const uint32_t T = prefix;                        // exactly `want` of the elements equal to T belong to the top k
    const uint32_t need_eq = want;

    // ---- (2) deterministic compaction: wave w owns columns [w * seg, (w + 1) * seg)
    const int seg = ((cols + TK_WAVES - 1) / TK_WAVES + 63) & ~63;
    const int c_begin = wave * seg, c_end = min(cols, c_begin + seg);
    uint32_t n_gt = 0, n_eq = 0;
    for (int c = c_begin + lane; c < c_begin + seg; c += 64) {
        const uint32_t key = c < c_end ? key_of(x[c]) : 0u;
        n_gt += __popcll(__ballot(c < c_end && key > T));
        n_eq += __popcll(__ballot(c < c_end && key == T));
    }
    if (lane == 0) { wave_gt[wave] = n_gt; wave_eq[wave] = n_eq; }
    __syncthreads();
    uint32_t base_gt = 0, base_eq = 0, total_gt = 0;
    for (int w = 0; w < TK_WAVES; ++w) {
        if (w < wave) { base_gt += wave_gt[w]; base_eq += wave_eq[w]; }
        total_gt += wave_gt[w];
    }
    // layout of cand: [0, total_gt) the elements above T, then the first need_eq elements equal to T in column order
    for (int c = c_begin + lane; c < c_begin + seg; c += 64) {
        const bool in = c < c_end;
        const uint32_t key = in ? key_of(x[c]) : 0u;
        const bool gt = in && key > T, eq = in && key == T;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long entry = ((unsigned long long)key << 32) | (uint32_t)(0xffffffffu - (uint32_t)c);
        if (gt) cand[base_gt + __popcll(bg & below)] = entry;
        if (eq) {
            const uint32_t pos = base_eq + __popcll(be & below);
            if (pos < need_eq) cand[total_gt + pos] = entry;
        }
        base_gt += __popcll(bg);
        base_eq += __popcll(be);
    }
    // pad to the next power of two with entries that sort last
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (int i = k + tid; i < n2; i += TK_THREADS) cand[i] = 0ull;
    __syncthreads();

    // ---- (3) bitonic sort, descending: larger key first, then smaller column (stored as 0xffffffff - column)
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (n2 >> 1); i += TK_THREADS) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long a = cand[lo], b = cand[hi];
                if ((a < b) == desc) { cand[lo] = b; cand[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += TK_THREADS) {
        const unsigned long long e = cand[i];
        out_val[(int64_t)blockIdx.x * k + i] = value_of((uint32_t)(e >> 32));
        out_idx[(int64_t)blockIdx.x * k + i] = (int64_t)(0xffffffffu - (uint32_t)e);
    }
}

// ---- joint re-ranking (get_image_knn_from_text_knn.py:59-92 + get_average_similarities.py:46-71 as one formula): for text
// neighbour j of query i, the image similarity is one dot product against a GATHERED train-image row, k rows of D floats per query
// (6.3 MB at k = 2048, D = 768) out of a table far larger than L2.  One 256-thread workgroup owns JS_BLOCK neighbours of one query:
// the query image row is staged in LDS once, every wave then walks its share of the neighbours RJ at a time - whole rows, one 16-byte
// load per lane and 256 columns, all loads of the RJ rows issued before the first use (D a multiple of 256 up to 1024: the row is
// unrolled, RJ = 4 rows = 4 D / 256 loads in flight per lane; any other D: RJ = 8 rows, one 256-column step at a time).  Every lane
// sums its own columns in column order and the 64 partial sums meet in the fixed butterfly of wave_sum: bitwise reproducible.
// An index outside its table never becomes an address: the row is replaced by row 0 of the table and its score by -inf.
constexpr int JS_BLOCK = 128, JS_WAVES = 4;

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
    acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); return fmaf(a.w, b.w, acc);
}

template <int NC>   // NC > 0: D == 256 NC
__global__ __launch_bounds__(64 * JS_WAVES) void joint_scores_kernel(int k, int D, int Ndq, int Ni, int Nqi, int blocks_per_query,
                                                                    const float* __restrict__ text_sim, const int64_t* __restrict__ text_idx,
                                                                    const int32_t* __restrict__ q2img, const float* __restrict__ train_img,
                                                                    int64_t ld_train, const float* __restrict__ query_img, int64_t ld_query,
                                                                    const int32_t* __restrict__ query_row, float* __restrict__ joint,
                                                                    float* __restrict__ img_sim) {
    extern __shared__ __attribute__((aligned(16))) float qs[];     // the query image row
    constexpr int RJ = NC > 0 ? 4 : 8;
    const int i = blockIdx.x / blocks_per_query, jb = (blockIdx.x - i * blocks_per_query) * JS_BLOCK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qr = query_row[i];
    const bool q_ok = qr >= 0 && qr < Nqi;
    const float* qrow = query_img + (int64_t)(q_ok ? qr : 0) * ld_query;
    for (int c = threadIdx.x * 4; c < D; c += 256 * 4) *reinterpret_cast<float4*>(qs + c) = *reinterpret_cast<const float4*>(qrow + c);
    __syncthreads();
    float4 qv[NC > 0 ? NC : 1];
    if constexpr (NC > 0) {
#pragma unroll
        for (int s = 0; s < NC; ++s) qv[s] = *reinterpret_cast<const float4*>(qs + s * 256 + lane * 4);
    }
    const int j_end = min(k, jb + JS_BLOCK);
    for (int j0 = jb + wave * RJ; j0 < j_end; j0 += JS_WAVES * RJ) {
        // lane r < RJ resolves neighbour j0 + r: its train image row, or -1
        int im = -1;
        if (lane < RJ && j0 + lane < j_end) {
            const int64_t ti = text_idx[(int64_t)i * k + j0 + lane];
            if (q_ok && ti >= 0 && ti < Ndq) {
                const int v = q2img[ti];
                if (v >= 0 && v < Ni) im = v;
            }
        }
        const float* rows[RJ];
#pragma unroll
        for (int r = 0; r < RJ; ++r) {
            const int v = __shfl(im, r, 64);
            rows[r] = train_img + (int64_t)(v < 0 ? 0 : v) * ld_train;
        }
        float acc[RJ];
#pragma unroll
        for (int r = 0; r < RJ; ++r) acc[r] = 0.f;
        if constexpr (NC > 0) {
            float4 t[RJ][NC];
#pragma unroll
            for (int r = 0; r < RJ; ++r)
#pragma unroll
                for (int s = 0; s < NC; ++s) t[r][s] = *reinterpret_cast<const float4*>(rows[r] + s * 256 + lane * 4);
#pragma unroll
            for (int r = 0; r < RJ; ++r)
#pragma unroll
                for (int s = 0; s < NC; ++s) acc[r] = dot4(qv[s], t[r][s], acc[r]);
        } else {
            for (int c = lane * 4; c < D; c += 256) {
                const float4 q4 = *reinterpret_cast<const float4*>(qs + c);
                float4 t[RJ];
#pragma unroll
                for (int r = 0; r < RJ; ++r) t[r] = *reinterpret_cast<const float4*>(rows[r] + c);
#pragma unroll
                for (int r = 0; r < RJ; ++r) acc[r] = dot4(q4, t[r], acc[r]);
            }
        }
        float mine = 0.f;                                      // lane r keeps the sum of neighbour j0 + r
#pragma unroll
        for (int r = 0; r < RJ; ++r) {
            const float s = wave_sum(acc[r]);
            if (lane == r) mine = s;
        }
        if (lane < RJ && j0 + lane < j_end) {
            const int64_t o = (int64_t)i * k + j0 + lane;
            const float sim = im >= 0 ? mine : -INFINITY;
            joint[o] = im >= 0 ? text_sim[o] + sim : -INFINITY;
            if (img_sim) img_sim[o] = sim;
        }
    }
}

}  // namespace

extern "C" int eavqa_l2_normalize_rows(int rows, int cols, float* x, int64_t ld, void* stream) {
    if (!x || rows <= 0 || cols <= 0 || ld < cols) return EAVQA_E_ARG;
    hipLaunchKernelGGL(l2_normalize_kernel, dim3(rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rows, cols, x, ld);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_topk_rows(int rows, int cols, const float* scores, int64_t ld, int k, float* out_val, int64_t* out_idx,
                               void* stream) {
    if (!scores || !out_val || !out_idx || rows <= 0 || cols <= 0 || ld < cols) return EAVQA_E_ARG;
    if (k <= 0 || k > TK_MAX || k > cols) return EAVQA_E_SHAPE;
    hipLaunchKernelGGL(topk_rows_kernel, dim3(rows), dim3(TK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), cols, scores, ld, k,
                       out_val, out_idx);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_rices_joint_scores(int Nq, int k, int D, int Ndq, int Ni, int Nqi, const float* text_sim, const int64_t* text_idx,
                                        const int32_t* q2img, const float* train_img, int64_t ld_train, const float* query_img,
                                        int64_t ld_query, const int32_t* query_row, float* joint, float* img_sim, void* stream) {
    if (!text_sim || !text_idx || !q2img || !train_img || !query_img || !query_row || !joint) return EAVQA_E_ARG;
    if (Nq <= 0 || k <= 0 || D <= 0 || Ndq <= 0 || Ni <= 0 || Nqi <= 0 || ld_train < D || ld_query < D) return EAVQA_E_ARG;
    if (k > TK_MAX || D % 4 || D > 16384) return EAVQA_E_SHAPE;
    if (ld_train % 4 || ld_query % 4 || !eavqa_aligned16(train_img) || !eavqa_aligned16(query_img)) return EAVQA_E_ALIGN;
    const int bpq = (k + JS_BLOCK - 1) / JS_BLOCK;
    if ((int64_t)Nq * bpq > 0x7fffffff) return EAVQA_E_SHAPE;
    const dim3 grid((unsigned)(Nq * bpq)), block(64 * JS_WAVES);
    const size_t lds = (size_t)D * 4;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define EAVQA_JS_ARGS k, D, Ndq, Ni, Nqi, bpq, text_sim, text_idx, q2img, train_img, ld_train, query_img, ld_query, query_row, joint, img_sim
    if (D == 256) hipLaunchKernelGGL(joint_scores_kernel<1>, grid, block, lds, s, EAVQA_JS_ARGS);
    else if (D == 512) hipLaunchKernelGGL(joint_scores_kernel<2>, grid, block, lds, s, EAVQA_JS_ARGS);
    else if (D == 768) hipLaunchKernelGGL(joint_scores_kernel<3>, grid, block, lds, s, EAVQA_JS_ARGS);
    else if (D == 1024) hipLaunchKernelGGL(joint_scores_kernel<4>, grid, block, lds, s, EAVQA_JS_ARGS);
    else hipLaunchKernelGGL(joint_scores_kernel<0>, grid, block, lds, s, EAVQA_JS_ARGS);
#undef EAVQA_JS_ARGS
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
