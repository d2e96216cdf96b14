// Sampling pick (eavqa_sample_pick in include/eavqa.h): HF's `_sample` step under TemperatureLogitsWarper -> TopKLogitsWarper ->
// TopPLogitsWarper for one decoder step, fused with the finished-row bookkeeping of greedy_pick_kernel (csrc/loss.hip).
//
// One 1024-thread workgroup per row.  The row is read from HBM once into registers (NPT values per thread, 16-byte loads when every
// row base is 16-byte aligned); every later pass runs over those registers.  Byte model: B * V * 4 read (+ B * V * 4 read again from L2
// and B * V * 4 written when `scores_out` is asked for).  At B = 32 a row per CU is latency bound: the time is the ~60 dependent
// bisection rounds (a few compares per held value, one wave butterfly, one barrier each), not the bytes.
//
// Layout: thread t holds the float4 chunks j = 0 .. NPT/4 - 1 at columns (j * 1024 + t) * 4 + e, so a wave's load is one contiguous
// 1 KiB and index order is (j, t, e).  Registers first hold the order-preserving 32-bit keys of s = logit / temperature (maximum and
// top-k threshold: bisection on the key, integer counts), then - in place - the bits of w = exp(s - max) of what top-k left (top-p
// threshold: bisection on the bits of w, which order like w for w >= 0; masses are fixed-order fp32 tree sums).
// Every sum is per-thread in register order, then a wave butterfly, then the 16 waves in order: bitwise reproducible, no float atomics.
#include "common.h"

namespace {

constexpr int SP_THREADS = 1024;
constexpr int SP_WAVES = SP_THREADS / EAVQA_WAVE;

// float -> uint32 whose unsigned order is the float order (-inf < finite < +inf); 0 is below every float that is not a NaN
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// s = logit / temperature as HF divides; a NaN holds no probability (-inf)
__device__ __forceinline__ float warp_temp(float x, float temperature) {
    const float s = x / temperature;
    return s != s ? -INFINITY : s;
}

// softmax weight of the value with key k: exp(s - max), exactly 1 at the maximum (also when that is +-inf)
__device__ __forceinline__ float weight(uint32_t k, uint32_t mxkey, float mx) { return k == mxkey ? 1.f : expf(key2f(k) - mx); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

// block-wide combine of one value per thread: wave butterfly, then the 16 wave results in order.  `slot` is one of two LDS rows used
// alternately by successive calls, so one barrier per call is enough (a row is rewritten two calls later, behind the next barrier).
template <typename T, typename WaveOp, typename Op>
__device__ __forceinline__ T block_combine(T v, T* slot, WaveOp wave_op, Op op) {
    v = wave_op(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = slot[0];
#pragma unroll
    for (int w = 1; w < SP_WAVES; ++w) r = op(r, slot[w]);
    return r;
}

struct Philox {
    // Philox4x32-10 (Salmon et al., SC'11; Random123 philox4x32_10): first output word for counter (c0, c1, c2, c3), key (k0, k1)
    static __device__ __forceinline__ uint32_t first_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
            const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
            c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        return c0;
    }
};

template <int NPT>
__global__ __launch_bounds__(SP_THREADS) void sample_pick_kernel(int V, const float* __restrict__ logits, int64_t ld, int vec, float temperature,
                                                                 int top_k, float top_p, uint64_t seed, uint64_t step, const float* uniform_in,
                                                                 float* uniform_out, int64_t pad, int64_t eos, int32_t* raw, int64_t* emitted,
                                                                 int64_t ld_emitted, int32_t* unfinished, float* logprob, float* scores_out,
                                                                 int64_t ld_scores, int vec_scores, int32_t* any_unfinished) {
    constexpr int NC = NPT / 4;                 // float4 chunks per thread
    __shared__ uint32_t su[2][SP_WAVES];
    __shared__ float sf[2][SP_WAVES];
    __shared__ float sseg[NC][SP_WAVES];
    __shared__ float seg[NC];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (int64_t)b * ld;
    int flip = 0;
    auto sum_u32 = [&](uint32_t v) { flip ^= 1; return block_combine(v, su[flip], wave_sum_u32, [](uint32_t a, uint32_t c) { return a + c; }); };
    auto max_u32 = [&](uint32_t v) { flip ^= 1; return block_combine(v, su[flip], wave_max_u32, [](uint32_t a, uint32_t c) { return max(a, c); }); };
    auto min_u32 = [&](uint32_t v) { flip ^= 1; return block_combine(v, su[flip], wave_min_u32, [](uint32_t a, uint32_t c) { return min(a, c); }); };
    auto sum_f32 = [&](float v) { flip ^= 1; return block_combine(v, sf[flip], wave_sum, [](float a, float c) { return a + c; }); };

    // ---- the one HBM read: keys of s = logit / temperature; columns >= V are never read and hold key 0 (below every real key)
    uint32_t r[NPT];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c0 = (j * SP_THREADS + tid) * 4;
        float v[4];
        if (vec && c0 + 3 < V) {
            const float4 q = *reinterpret_cast<const float4*>(x + c0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = c0 + e < V ? x[c0 + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) r[j * 4 + e] = __float_as_uint(v[e]);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        __builtin_amdgcn_sched_barrier(0);      // chunk by chunk: interleaving all NPT divisions costs more registers than there are
        const int c0 = (j * SP_THREADS + tid) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[j * 4 + e] = c0 + e < V ? f2key(warp_temp(__uint_as_float(r[j * 4 + e]), temperature)) : 0u;
    }

    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) mine = max(mine, r[i]);
    const uint32_t mxkey = max_u32(mine);
    const float mx = key2f(mxkey);

    // ---- top-k: the key of the top_k-th largest value = the largest K with count(key >= K) >= top_k; ties with it are all kept
    uint32_t thr_key = 1u;
    if (top_k > 0 && top_k < V) {
        uint32_t K = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = K | (1u << bit);
            uint32_t n = 0;
#pragma unroll
            for (int i = 0; i < NPT; ++i) n += r[i] >= cand ? 1u : 0u;
            if (sum_u32(n) >= (uint32_t)top_k) K = cand;
        }
        thr_key = K;
    }

    // ---- weights in place: w = exp(s - max) of what top-k left (exactly 1 at the maximum, also when that is +-inf), 0 for the rest
    float zt = 0.f;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const uint32_t k = r[i];
        const float w = k >= thr_key ? weight(k, mxkey, mx) : 0.f;
        r[i] = __float_as_uint(w);
        zt += w;
    }
    const float Z = sum_f32(zt);

    // ---- top-p: HF removes, in ascending order, while the cumulative probability is <= 1 - top_p.  As a threshold on w: the largest
    // bit pattern T with mass(w < T) <= (1 - top_p) * Z; everything with w >= T stays (the maximum always does)
    uint32_t thr_w = 0u;
    float Zk = Z;
    if (top_p < 1.f) {
        const float limit = (1.f - top_p) * Z;
        uint32_t T = 0;
        for (int bit = 29; bit >= 0; --bit) {            // w <= 1 = 0x3F800000 < 2^30
            const uint32_t cand = T | (1u << bit);
            float m = 0.f;
#pragma unroll
            for (int i = 0; i < NPT; ++i) m += r[i] < cand ? __uint_as_float(r[i]) : 0.f;
            if (sum_f32(m) <= limit) T = cand;
        }
        thr_w = min(T, 0x3F800000u);
        float zk = 0.f;
#pragma unroll
        for (int i = 0; i < NPT; ++i) zk += r[i] >= thr_w ? __uint_as_float(r[i]) : 0.f;
        Zk = sum_f32(zk);
    }

    // ---- processed scores (HF's `.scores` under sampling): s where kept, -inf where removed.  A rolled loop over a second read of the
    // row (L2) that recomputes s and w with the expressions above: indexing the register copy would need every chunk unrolled with a
    // second set of NPT values in flight, which does not fit beside the first
    if (scores_out) {
        float* so = scores_out + (int64_t)b * ld_scores;
        const float* xs = x;
        asm volatile("" : "+s"(xs));             // a read of its own: otherwise all NPT values of s stay alive from the first one
        for (int c0 = tid * 4; c0 < V; c0 += SP_THREADS * 4) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float s = warp_temp(c0 + e < V ? xs[c0 + e] : 0.f, temperature);
                const uint32_t k = f2key(s);
                const bool keep = (k >= thr_key) & (__float_as_uint(weight(k, mxkey, mx)) >= thr_w);
                o[e] = keep ? s : -INFINITY;
            }
            if (vec_scores && c0 + 3 < V) *reinterpret_cast<float4*>(so + c0) = make_float4(o[0], o[1], o[2], o[3]);
            else
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + e < V) so[c0 + e] = o[e];
        }
    }

    // ---- the draw: smallest index i (order (j, t, e)) whose inclusive kept mass exceeds u * Zk
    float u;
    if (uniform_in) u = uniform_in[b];
    else u = (float)(Philox::first_word((uint32_t)step, (uint32_t)(step >> 32), (uint32_t)b, 0u, (uint32_t)seed, (uint32_t)(seed >> 32)) >> 8) * 0x1p-24f;
    const float target = u * Zk;

    // per-thread mass of each chunk, then the mass of each 4096-column segment j (all NC segment sums share one barrier)
    float pj[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { r[j * 4 + e] = r[j * 4 + e] >= thr_w ? r[j * 4 + e] : 0u; a += __uint_as_float(r[j * 4 + e]); }
        pj[j] = a;
        const float ws = wave_sum(a);
        if ((tid & 63) == 0) sseg[j][tid >> 6] = ws;
    }
    __syncthreads();
    if (tid < NC) {
        float a = sseg[tid][0];
#pragma unroll
        for (int w = 1; w < SP_WAVES; ++w) a += sseg[tid][w];
        seg[tid] = a;
    }
    __syncthreads();
    // the segment: the first whose running total passes the target; rounding (or a `u` outside [0, 1)) may leave none - then the last
    // segment that holds mass.  Only entries with mass > 0 are ever chosen, here and below, so a removed token is never drawn.
    int jstar = -1, jlast = 0;
    float base = 0.f, run = 0.f;
    for (int j = 0; j < NC; ++j) {
        const float sj = seg[j];
        if (sj > 0.f) {
            jlast = j;
            if (jstar < 0 && run + sj > target) { jstar = j; base = run; }
        }
        run += sj;
    }
    if (jstar < 0) { jstar = jlast; base = -INFINITY; }     // then no thread passes the target either: the last one with mass owns the draw
    float own = 0.f;
    uint32_t own_w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (j == jstar) {
            own = pj[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) own_w[e] = r[j * 4 + e];
        }
    // scan of the per-thread sums in thread order: inclusive within the wave (Hillis-Steele), waves in order
    float incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o, 64);
        if ((tid & 63) >= o) incl += up;
    }
    flip ^= 1;
    if ((tid & 63) == 63) sf[flip][tid >> 6] = incl;
    __syncthreads();
    float wbase = base;
    for (int w = 0; w < (tid >> 6); ++w) wbase += sf[flip][w];
    const float excl_in_wave = __shfl_up(incl, 1, 64);
    const float excl = wbase + ((tid & 63) ? excl_in_wave : 0.f);
    // owner: the first thread with mass whose inclusive total passes the target; else the last thread with mass
    const bool pass = own > 0.f && wbase + incl > target;
    const uint32_t code = min_u32(pass ? (uint32_t)tid : own > 0.f ? 4096u - (uint32_t)tid : 8192u);
    const int owner = code < 1024u ? (int)code : code < 8192u ? (int)(4096u - code) : 0;
    if (tid != owner) return;

    int e_pick = 0;
    {
        float acc = excl;
        bool found = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float w = __uint_as_float(own_w[e]);
            if (!found && w > 0.f) {
                e_pick = e;
                acc += w;
                found = acc > target;
            }
        }
    }
    int tok = (jstar * SP_THREADS + tid) * 4 + e_pick;
    tok = tok < V ? tok : V - 1;                            // unreachable (columns >= V hold no mass); keeps the index in [0, V) regardless
    float w_pick = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) w_pick = e == e_pick ? __uint_as_float(own_w[e]) : w_pick;

    raw[b] = tok;
    int64_t em = tok;
    if (eos >= 0) {                                         // as greedy_pick_kernel: finished rows emit pad
        const int un = unfinished[b];
        em = un ? (int64_t)tok : pad;
        const int un2 = un * (em != eos ? 1 : 0);
        unfinished[b] = un2;
        if (any_unfinished && un2) atomicOr(any_unfinished, 1);
    }
    emitted[(int64_t)b * ld_emitted] = em;
    if (logprob) logprob[b] = logf(w_pick) - logf(Zk);
    if (uniform_out) uniform_out[b] = u;
}

}  // namespace

extern "C" int eavqa_sample_pick(int B, int V, const float* logits, int64_t ld, float temperature, int top_k, float top_p, uint64_t seed,
                                 uint64_t step, const float* uniform_in, float* uniform_out, int64_t pad_token_id, int64_t eos_token_id,
                                 int32_t* raw, int64_t* emitted, int64_t ld_emitted, int32_t* unfinished, float* logprob, float* scores_out,
                                 int64_t ld_scores, int32_t* any_unfinished, void* stream) {
    if (B <= 0 || V <= 0 || !logits || !raw || !emitted) return EAVQA_E_ARG;
    if (eos_token_id >= 0 && !unfinished) return EAVQA_E_ARG;
    if (ld < V || (scores_out && ld_scores < V)) return EAVQA_E_ARG;
    if (!(temperature > 0.f) || !(temperature <= FLT_MAX)) return EAVQA_E_ARG;
    if (!(top_p > 0.f)) return EAVQA_E_ARG;                 // also a NaN
    if (V > 65536) return EAVQA_E_SHAPE;
    const int vec = eavqa_aligned16(logits) && ld % 4 == 0;
    const int vec_scores = scores_out && eavqa_aligned16(scores_out) && ld_scores % 4 == 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define EAVQA_SAMPLE_LAUNCH(NPT)                                                                                                            \
    hipLaunchKernelGGL(sample_pick_kernel<NPT>, dim3(B), dim3(SP_THREADS), 0, s, V, logits, ld, vec, temperature, top_k, top_p, seed, step, \
                       uniform_in, uniform_out, pad_token_id, eos_token_id, raw, emitted, ld_emitted, unfinished, logprob, scores_out,      \
                       ld_scores, vec_scores, any_unfinished)
    if (V <= 8 * SP_THREADS) EAVQA_SAMPLE_LAUNCH(8);
    else if (V <= 32 * SP_THREADS) EAVQA_SAMPLE_LAUNCH(32);
    else EAVQA_SAMPLE_LAUNCH(64);
#undef EAVQA_SAMPLE_LAUNCH
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
