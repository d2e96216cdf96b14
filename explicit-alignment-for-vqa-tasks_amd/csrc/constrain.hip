// Decoding inside a closed answer set (eavqa_trie_constrain in include/eavqa.h): HF's PrefixConstrainedLogitsProcessor
// (transformers/generation/logits_process.py:1484-1553, 5.15) for the callback "the allowed next ids are the children of the trie node
// the generated ids lead to, plus eos where a member of the set ends; [eos] once the row has ended or left the set", for one decoder
// step, in place on the float32 score rows.
//
// One 1024-thread workgroup per row, three phases:
//   walk        the row's generated ids history[prompt_len : cur_len] from the item's root, one binary search per id over the node's
//               sorted child list.  STATELESS: redone from the history every step, so a beam reorder needs no bookkeeping; the depth is
//               bounded by the longest member of the set (the walk stops at the first id that is no child, eos included - eos is never a
//               child).  Every thread walks on its own: the loads are the same addresses across the workgroup (one L2 line each), and no
//               barrier or LDS broadcast is needed.
//   stage       the final node's child list -> LDS when it holds at most TC_LDS_CHILDREN ids (8 KB); a larger fan-out is searched where
//               it lies, in global memory.
//   write       every thread takes its 4 consecutive columns per pass: ONE lower bound into the sorted list, then a merge over the 4
//               columns.  Without `to_logprobs` the row is never read: a group with no allowed column is one 16-byte store of -inf, a group
//               with one writes only its other columns - at most R * V * 4 bytes.  With `to_logprobs` the row is first reduced by
//               row_max_lse (csrc/row_lse.h), then read again and written as (x - M) - lse or -inf, so an allowed column holds the bits
//               eavqa_logits_process(to_logprobs = 1) would leave.  A thread reads only the columns it writes itself: no thread depends
//               on another's global store.
// Columns >= V are neither read nor written.  Every index taken from the CSR arrays is checked against [0, n_nodes) / [0, n_edges]
// before it is used, so neither the history nor a damaged table can send a load outside them.
#include "common.h"
#include "row_lse.h"

namespace {

constexpr int TC_LDS_CHILDREN = 2048;          // child ids staged in LDS (8 KB of the workgroup's 64 KB); eavqa.h names the bound

template <bool LOGPROBS>
__global__ __launch_bounds__(BR_THREADS) void trie_constrain_kernel(int V, float* scores, int64_t ld, const int64_t* __restrict__ history,
                                                                    int64_t ld_history, int prompt_len, int cur_len, int eos,
                                                                    const int32_t* __restrict__ child_begin, const int32_t* __restrict__ child_tok,
                                                                    const int32_t* __restrict__ child_node, const uint8_t* __restrict__ is_end,
                                                                    int n_nodes, int n_edges, const int32_t* __restrict__ roots,
                                                                    int rows_per_item) {
    __shared__ int32_t s_tok[TC_LDS_CHILDREN];
    __shared__ float s_m[BR_WAVES], s_s[BR_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    float* x = scores + (int64_t)row * ld;
    const bool vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15u) == 0);

    // ---- walk: `on` = the generated ids are a path of the trie and `node` is where it ends
    int node = roots ? roots[row / rows_per_item] : 0;
    bool on = node >= 0 && node < n_nodes;
    int begin = 0, end = 0;
    auto children = [&](int nd) {
        begin = min(max(child_begin[nd], 0), n_edges);
        end = min(max(child_begin[nd + 1], begin), n_edges);
    };
    if (on) children(node);
    const int64_t* h = history + (int64_t)row * ld_history;
    for (int j = prompt_len; on && j < cur_len; ++j) {
        const int64_t tok = h[j];
        int lo = begin, hi = end;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)child_tok[mid] < tok) lo = mid + 1;
            else hi = mid;
        }
        on = lo < end && (int64_t)child_tok[lo] == tok;
        if (on) {
            node = child_node[lo];
            on = node >= 0 && node < n_nodes;
        }
        if (on) children(node);
    }
    // off the trie (or ended: eos is no child): only eos.  A node without children allows eos whatever is_end says, so no row is left empty
    const int n = on ? end - begin : 0;
    const bool eos_ok = !on || n == 0 || is_end[node] != 0;
    const int32_t* list = child_tok + begin;

    float M = 0.f, lse = 0.f;
    if constexpr (LOGPROBS) row_max_lse(x, V, vec, s_m, s_s, M, lse, [](const float*, int) {});

    // ---- stage (n is the same in every thread of the workgroup, so the barrier is reached by all or by none)
    const bool lds = n <= TC_LDS_CHILDREN;
    if (lds && n > 0) {
        for (int i = tid; i < n; i += BR_THREADS) s_tok[i] = list[i];
        __syncthreads();
    }
    auto tok_at = [&](int i) { return lds ? s_tok[i] : list[i]; };

    // ---- write
    for (int c0 = tid * 4; c0 < V; c0 += BR_THREADS * 4) {
        int lo = 0, hi = n;                                             // first child id >= c0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tok_at(mid) < c0) lo = mid + 1;
            else hi = mid;
        }
        bool keep[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            while (lo < n && tok_at(lo) < c) ++lo;                      // (a repeated id in the list: skipped)
            keep[j] = (lo < n && tok_at(lo) == c) || (eos_ok && c == eos);
            any = any || keep[j];
        }
        if constexpr (LOGPROBS) {
            float v[4];
            load4(x, c0, V, vec, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = keep[j] ? (v[j] - M) - lse : -INFINITY;
            if (vec && c0 + 3 < V) *reinterpret_cast<float4*>(x + c0) = make_float4(v[0], v[1], v[2], v[3]);
            else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < V) x[c0 + j] = v[j];
        } else {
            if (!any && vec && c0 + 3 < V) *reinterpret_cast<float4*>(x + c0) = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!keep[j] && c0 + j < V) x[c0 + j] = -INFINITY;
        }
    }
}

}  // namespace

extern "C" int eavqa_trie_constrain(int R, int V, float* scores, int64_t ld, int to_logprobs, const int64_t* history, int64_t ld_history,
                                    int prompt_len, int cur_len, int64_t eos_token_id, const int32_t* child_begin, const int32_t* child_tok,
                                    const int32_t* child_node, const uint8_t* is_end, int n_nodes, int n_edges, const int32_t* roots,
                                    int rows_per_item, void* stream) {
    if (R <= 0 || V <= 0 || !scores || cur_len < 0 || prompt_len < 0 || prompt_len > cur_len) return EAVQA_E_ARG;
    if (cur_len > prompt_len && !history) return EAVQA_E_ARG;
    if (to_logprobs != 0 && to_logprobs != 1) return EAVQA_E_ARG;
    if (eos_token_id < 0 || eos_token_id >= V) return EAVQA_E_ARG;      // eos is what keeps every row non-empty
    if (n_nodes < 1 || n_edges < 0 || !child_begin || !is_end || (n_edges > 0 && (!child_tok || !child_node))) return EAVQA_E_ARG;
    if (rows_per_item < 1) return EAVQA_E_ARG;
    if (ld < V || (cur_len > prompt_len && ld_history < cur_len)) return EAVQA_E_SHAPE;
    if (R % rows_per_item != 0) return EAVQA_E_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (to_logprobs)
        hipLaunchKernelGGL(trie_constrain_kernel<true>, dim3(R), dim3(BR_THREADS), 0, s, V, scores, ld, history, ld_history, prompt_len, cur_len,
                           (int)eos_token_id, child_begin, child_tok, child_node, is_end, n_nodes, n_edges, roots, rows_per_item);
    else
        hipLaunchKernelGGL(trie_constrain_kernel<false>, dim3(R), dim3(BR_THREADS), 0, s, V, scores, ld, history, ld_history, prompt_len, cur_len,
                           (int)eos_token_id, child_begin, child_tok, child_node, is_end, n_nodes, n_edges, roots, rows_per_item);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
