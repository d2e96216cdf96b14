// Fused AdamW over one flat float32 parameter buffer (eavqa_adamw in include/eavqa.h).
// HBM-bound: per element 16 B read (param, grad, m, v) + 12 B written (+ 2 B bf16 shadow).
// Gradient-norm clipping and the non-finite guard (eavqa_grad_sumsq, eavqa_clip_plan, eavqa_adamw_clipped): one more 4 B / element read
// of the gradient, a 32-byte state block on the device, and the same update with its three step scalars read from that block.
#include "common.h"

namespace {

// Geometry of adamw_kernel / adamw_clipped_kernel: at most ONE 256-thread workgroup per CU (one wave per SIMD, 126 of its 512 VGPRs, no
// LDS), each thread with ADAMW_UNROLL grid strides = 16 16-byte loads in flight (64 KiB per CU).  The update is HBM-bound and needs
// no more residency than that to stream (faster alone than the grid that filled every wave slot); what it leaves
// free - 28 of 32 wave slots, three quarters of the registers, all of the LDS - is open to the side stream's workgroups while it runs
// (which of the CLIP tower's fit there: profiles/adamw_tower_overlap.md).  Its registers also cap it at four waves per SIMD wherever the
// workgroups land.  One trip of the capped grid covers ADAMW_MAX_BLOCKS * ADAMW_THREADS * ADAMW_UNROLL float4.
constexpr int ADAMW_THREADS = 256;
constexpr int ADAMW_UNROLL = 4;
constexpr int ADAMW_MAX_BLOCKS = 256;

// param, grad, m, v and the shadow are each touched once per launch and are far larger than the caches: streamed past them.
__device__ __forceinline__ float4 stream_ld4(const float4* q) {
    const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q));
    return make_float4(t[0], t[1], t[2], t[3]);
}
__device__ __forceinline__ void stream_st4(float4* q, const float4 x) {
    f32x4 t;
    t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(q));
}
__device__ __forceinline__ void stream_st4(float* q, const float4 x) { stream_st4(reinterpret_cast<float4*>(q), x); }
__device__ __forceinline__ void stream_st4(bf16_t* q, const float4 x) {
    bf16x4 t;
    t[0] = (bf16_t)x.x; t[1] = (bf16_t)x.y; t[2] = (bf16_t)x.z; t[3] = (bf16_t)x.w;
    __builtin_nontemporal_store(t, reinterpret_cast<bf16x4*>(q));
}

// The whole update of adamw_kernel / adamw_clipped_kernel: one body, so both kernels evaluate the same expressions in the same order
// (eavqa_adamw_clipped is bit-equal to eavqa_adamw whenever the three scalars are).
template <typename S, bool HAS_SHADOW>
__device__ __forceinline__ void adamw_body(int64_t n4, int64_t n, float* param, const float* grad, float* m, float* v,
                                           float lr, float beta1, float beta2, float eps, float decay_mul,
                                           float inv_bc1, float inv_sqrt_bc2, float grad_scale, S* shadow, const int64_t first,
                                           const int64_t stride, const unsigned block_threads) {
    auto update = [&](float4& p, const float4 g, float4& mm, float4& vv) {
        float pa[4] = {p.x, p.y, p.z, p.w}, ga[4] = {g.x, g.y, g.z, g.w};
        float ma[4] = {mm.x, mm.y, mm.z, mm.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
        // p *= 1 - lr*wd (decoupled decay first); m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g g; p -= lr/bc1 * m / denom.
        // Which product of each sum is folded into the fused multiply-add decides the last bit, so it is written out and not left to
        // the compiler's contraction (which changes with the loop around it): these are the roundings every earlier build produced.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
            const float gj = ga[j] * grad_scale;
            ma[j] = __builtin_fmaf(1.f - beta1, gj, beta1 * ma[j]);
            va[j] = __builtin_fmaf(gj, (1.f - beta2) * gj, beta2 * va[j]);
            const float denom = __builtin_fmaf(sqrtf(va[j]), inv_sqrt_bc2, eps);
            pa[j] = __builtin_fmaf(pa[j], decay_mul, -((lr * inv_bc1) * (ma[j] / denom)));
        }
        p = make_float4(pa[0], pa[1], pa[2], pa[3]);
        mm = make_float4(ma[0], ma[1], ma[2], ma[3]);
        vv = make_float4(va[0], va[1], va[2], va[3]);
    };
    // U grid strides per iteration: 4 U 16-byte loads in flight per thread before the first use (the update is element-wise, so the
    // order in which elements are visited does not change any result)
    constexpr int U = ADAMW_UNROLL;
    float4* const p4 = reinterpret_cast<float4*>(param);
    const float4* const g4 = reinterpret_cast<const float4*>(grad);
    float4* const m4 = reinterpret_cast<float4*>(m);
    float4* const v4 = reinterpret_cast<float4*>(v);
    // Every address is a workgroup-uniform 64-bit base plus the lane's 32-bit offset.  A stride that starts past the end reads the
    // trip's first one again, a lane past the end reads its stride's first float4: in bounds, unused.
    const unsigned lane = threadIdx.x;
    for (int64_t b = first; b < n4; b += U * stride) {
        int64_t base[U];
        unsigned off[U];
        bool on[U];
        float4 p[U], g[U], mm[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t bu = b + u * stride;
            base[u] = bu < n4 ? bu : b;
            on[u] = bu < n4 && (int64_t)lane < n4 - bu;
            off[u] = on[u] ? lane : 0u;
            p[u] = stream_ld4(p4 + base[u] + off[u]);
            g[u] = stream_ld4(g4 + base[u] + off[u]);
            mm[u] = stream_ld4(m4 + base[u] + off[u]);
            vv[u] = stream_ld4(v4 + base[u] + off[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (on[u]) {
                update(p[u], g[u], mm[u], vv[u]);
                stream_st4(p4 + base[u] + off[u], p[u]);
                stream_st4(m4 + base[u] + off[u], mm[u]);
                stream_st4(v4 + base[u] + off[u], vv[u]);
                if (HAS_SHADOW) stream_st4(shadow + 4 * base[u] + 4 * off[u], p[u]);
            }
        }
    }
    // tail (n not a multiple of 4).  Left to the compiler, these sums came out with the float4 path's roundings only beside an fp32
    // shadow; beside no shadow or a bf16 one v and p were unfused and m folded its other product.  Written out as they came out, for
    // the same reason: a buffer keeps its bits whatever build updates it.
    constexpr bool TAIL_AS_BODY = HAS_SHADOW && sizeof(S) == sizeof(float);
    if (blockIdx.x == 0) {
        for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += block_threads) {
#pragma clang fp contract(off)
            const float gj = grad[i] * grad_scale;
            float pj, mj, vj;
            if (TAIL_AS_BODY) {
                mj = __builtin_fmaf(1.f - beta1, gj, beta1 * m[i]);
                vj = __builtin_fmaf(gj, (1.f - beta2) * gj, beta2 * v[i]);
                pj = __builtin_fmaf(param[i], decay_mul, -((lr * inv_bc1) * (mj / __builtin_fmaf(sqrtf(vj), inv_sqrt_bc2, eps))));
            } else {
                mj = __builtin_fmaf(beta1, m[i], (1.f - beta1) * gj);
                vj = beta2 * v[i] + (1.f - beta2) * gj * gj;
                pj = param[i] * decay_mul - (lr * inv_bc1) * (mj / __builtin_fmaf(sqrtf(vj), inv_sqrt_bc2, eps));
            }
            param[i] = pj; m[i] = mj; v[i] = vj;
            if (HAS_SHADOW) elem<S>::st(shadow + i, pj);
        }
    }
}

template <typename S, bool HAS_SHADOW>
__global__ __launch_bounds__(ADAMW_THREADS) void adamw_kernel(int64_t n4, int64_t n, float* param, const float* grad, float* m, float* v,
                                                    float lr, float beta1, float beta2, float eps, float decay_mul,
                                                    float inv_bc1, float inv_sqrt_bc2, float grad_scale, S* shadow) {
    adamw_body<S, HAS_SHADOW>(n4, n, param, grad, m, v, lr, beta1, beta2, eps, decay_mul, inv_bc1, inv_sqrt_bc2, grad_scale, shadow,
                              (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, blockDim.x);
}

// The same update with grad_scale and the bias corrections read from the state block eavqa_clip_plan wrote earlier on the stream.  A
// skipped step returns before any store: param, m, v and the shadow keep their bits.
template <typename S, bool HAS_SHADOW>
__global__ __launch_bounds__(ADAMW_THREADS) void adamw_clipped_kernel(int64_t n4, int64_t n, float* param, const float* grad, float* m, float* v,
                                                            float lr, float beta1, float beta2, float eps, float decay_mul,
                                                            const eavqa_clip_state_t* state, S* shadow) {
    if (state->skip) return;
    adamw_body<S, HAS_SHADOW>(n4, n, param, grad, m, v, lr, beta1, beta2, eps, decay_mul, state->inv_bc1, state->inv_sqrt_bc2,
                              state->scale_eff, shadow, (int64_t)blockIdx.x * blockDim.x, (int64_t)gridDim.x * blockDim.x, blockDim.x);
}

// ---- sum of squares of the flat gradient -------------------------------------------------------------------------------------------
constexpr int SUMSQ_THREADS = 256;
constexpr int SUMSQ_LOADS = 4;                                   // 16-byte loads in flight per thread
constexpr int64_t SUMSQ_SLICE = 2 * SUMSQ_LOADS * SUMSQ_THREADS;  // float4 per workgroup below the cap: two trips of the load loop
constexpr int SUMSQ_MAX_PARTIALS = 2048;

// Workgroup b owns the float4 [b * per, min((b + 1) * per, n4)), per = ceil(n4 / P); thread t takes t, t + 256, ... of it, four loads
// per trip.  The square of a float is exact in double, so every thread's sum is a plain chain of double additions in index order;
// lanes combine by the xor butterfly, the four waves in wave order: a fixed order, the same bits on every run.
__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_kernel(int64_t n4, int64_t n, const float* grad, double* partials) {
    const int64_t per = (n4 + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n4 ? lo + per : n4;
    const float4* g4 = reinterpret_cast<const float4*>(grad);
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += SUMSQ_LOADS * SUMSQ_THREADS) {
        float4 a[SUMSQ_LOADS];
#pragma unroll
        for (int u = 0; u < SUMSQ_LOADS; ++u) {
            const int64_t j = i + u * SUMSQ_THREADS;
            a[u] = j < hi ? g4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < SUMSQ_LOADS; ++u) {
            acc += (double)a[u].x * (double)a[u].x;
            acc += (double)a[u].y * (double)a[u].y;
            acc += (double)a[u].z * (double)a[u].z;
            acc += (double)a[u].w * (double)a[u].w;
        }
    }
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) {
        const double t = (double)grad[n4 * 4 + threadIdx.x];
        acc += t * t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double wave_part[SUMSQ_THREADS / EAVQA_WAVE];
    if ((threadIdx.x & (EAVQA_WAVE - 1)) == 0) wave_part[threadIdx.x / EAVQA_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_part[0];
#pragma unroll
        for (int w = 1; w < SUMSQ_THREADS / EAVQA_WAVE; ++w) s += wave_part[w];
        partials[blockIdx.x] = s;
    }
}

// One workgroup: the partials staged through LDS, then added by one thread in index order.
__global__ __launch_bounds__(256) void clip_plan_kernel(const double* partials, int P, float pre_scale, float max_norm, const float2* bc,
                                                        int bc_len, eavqa_clip_state_t* st) {
    __shared__ double sh[SUMSQ_MAX_PARTIALS];
    for (int i = threadIdx.x; i < P; i += blockDim.x) sh[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < P; ++i) s += sh[i];
    const float norm = (float)((double)pre_scale * sqrt(s));
    st->norm = norm;
    if (isfinite(norm)) {
        const int t = st->applied_steps + 1;
        const int row = (t < bc_len ? t : bc_len) - 1;
        const float2 c = bc[row > 0 ? row : 0];
        const float coef = fminf(1.f, max_norm / (norm + 1e-6f));
        st->scale_eff = pre_scale * coef;
        st->inv_bc1 = c.x;
        st->inv_sqrt_bc2 = c.y;
        st->applied_steps = t;
        st->skip = 0;
    } else {
        st->scale_eff = 0.f;
        st->skipped_steps = st->skipped_steps + 1;
        st->skip = 1;
    }
}

inline int adamw_blocks(int64_t n4) {
    int blocks = (int)((n4 + ADAMW_THREADS - 1) / ADAMW_THREADS);
    if (blocks > ADAMW_MAX_BLOCKS) blocks = ADAMW_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    return blocks;
}

}  // namespace

static_assert(sizeof(eavqa_clip_state_t) == 32, "eavqa_clip_state_t is 32 bytes");

extern "C" int eavqa_adamw(int64_t n, float* param, const float* grad, float* m, float* v, int step, float lr, float beta1,
                           float beta2, float eps, float weight_decay, float grad_scale, int shadow_dtype, void* shadow,
                           void* stream) {
    if (n <= 0 || !param || !grad || !m || !v || step < 1) return EAVQA_E_ARG;
    if (!eavqa_aligned16(param) || !eavqa_aligned16(grad) || !eavqa_aligned16(m) || !eavqa_aligned16(v)) return EAVQA_E_ALIGN;
    // bias corrections in double on the host, as torch does with Python floats
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float inv_bc1 = (float)(1.0 / bc1);
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    const float decay_mul = (float)(1.0 - (double)lr * (double)weight_decay);
    const int64_t n4 = n / 4;
    const int blocks = adamw_blocks(n4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define EAVQA_ADAMW(S, HAS)                                                                                                    \
    hipLaunchKernelGGL((adamw_kernel<S, HAS>), dim3(blocks), dim3(ADAMW_THREADS), 0, s, n4, n, param, grad, m, v, lr, beta1, \
                       beta2, eps, decay_mul, inv_bc1, inv_sqrt_bc2, grad_scale, reinterpret_cast<S*>(shadow))
    if (!shadow) EAVQA_ADAMW(float, false);
    else if (shadow_dtype == EAVQA_BF16) EAVQA_ADAMW(bf16_t, true);
    else if (shadow_dtype == EAVQA_F32) EAVQA_ADAMW(float, true);
    else return EAVQA_E_DTYPE;
#undef EAVQA_ADAMW
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_grad_sumsq_partials(int64_t n) {
    if (n <= 0) return 0;
    const int64_t p = (n / 4 + SUMSQ_SLICE - 1) / SUMSQ_SLICE;
    return p < 1 ? 1 : p > SUMSQ_MAX_PARTIALS ? SUMSQ_MAX_PARTIALS : (int)p;
}

extern "C" int eavqa_grad_sumsq(int64_t n, const float* grad, double* partials, int P, void* stream) {
    if (n <= 0 || !grad || !partials || P != eavqa_grad_sumsq_partials(n)) return EAVQA_E_ARG;
    if (!eavqa_aligned16(grad) || (reinterpret_cast<uintptr_t>(partials) & 7u)) return EAVQA_E_ALIGN;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(P), dim3(SUMSQ_THREADS), 0, reinterpret_cast<hipStream_t>(stream), n / 4, n, grad, partials);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_clip_plan(const double* partials, int P, float pre_scale, float max_norm, const float* bc_table, int bc_len,
                               eavqa_clip_state_t* state, void* stream) {
    if (!partials || !bc_table || !state || P < 1 || P > SUMSQ_MAX_PARTIALS || bc_len < 1) return EAVQA_E_ARG;
    if (!(pre_scale > 0.f) || !(pre_scale <= FLT_MAX) || !(max_norm > 0.f)) return EAVQA_E_ARG;      // (NaN fails every comparison)
    if ((reinterpret_cast<uintptr_t>(partials) & 7u) || (reinterpret_cast<uintptr_t>(bc_table) & 7u) || !eavqa_aligned16(state))
        return EAVQA_E_ALIGN;
    hipLaunchKernelGGL(clip_plan_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), partials, P, pre_scale, max_norm,
                       reinterpret_cast<const float2*>(bc_table), bc_len, state);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_adamw_clipped(int64_t n, float* param, const float* grad, float* m, float* v, float lr, float beta1, float beta2,
                                   float eps, float weight_decay, const eavqa_clip_state_t* state, int shadow_dtype, void* shadow,
                                   void* stream) {
    if (n <= 0 || !param || !grad || !m || !v || !state) return EAVQA_E_ARG;
    if (!eavqa_aligned16(param) || !eavqa_aligned16(grad) || !eavqa_aligned16(m) || !eavqa_aligned16(v) || !eavqa_aligned16(state))
        return EAVQA_E_ALIGN;
    const float decay_mul = (float)(1.0 - (double)lr * (double)weight_decay);
    const int64_t n4 = n / 4;
    const int blocks = adamw_blocks(n4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define EAVQA_ADAMW_CLIPPED(S, HAS)                                                                                          \
    hipLaunchKernelGGL((adamw_clipped_kernel<S, HAS>), dim3(blocks), dim3(ADAMW_THREADS), 0, s, n4, n, param, grad, m, v, lr, \
                       beta1, beta2, eps, decay_mul, state, reinterpret_cast<S*>(shadow))
    if (!shadow) EAVQA_ADAMW_CLIPPED(float, false);
    else if (shadow_dtype == EAVQA_BF16) EAVQA_ADAMW_CLIPPED(bf16_t, true);
    else if (shadow_dtype == EAVQA_F32) EAVQA_ADAMW_CLIPPED(float, true);
    else return EAVQA_E_DTYPE;
#undef EAVQA_ADAMW_CLIPPED
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
