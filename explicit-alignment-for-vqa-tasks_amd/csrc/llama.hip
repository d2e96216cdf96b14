// Llama-family kernels (include/eavqa_llama.h, "Llama-family frozen causal LM"): rotary position embedding on QKV rows and its fused
// split-K finish, the SwiGLU gate forward / backward and its split-K finish.  All four are HBM-bound elementwise passes; SiLU lives
// here and not in common.h's act_fwd / act_bwd, so no other kernel's code changes.
#include <algorithm>
#include "common.h"
#include "eavqa_llama.h"

namespace {
// silu(g) = g sigmoid(g);  silu'(g) = s (1 + g (1 - s))
__device__ __forceinline__ float silu(float g) { return g * fast_sigmoid(g); }
__device__ __forceinline__ float silu_grad(float g) {
    const float s = fast_sigmoid(g);
    return s * (1.f + g * (1.f - s));
}

// (a, b) -> (a c - b s, b c + a s): float32, each output one product pair and one sum
__device__ __forceinline__ void rotate4(float4& a, float4& b, const float4 c, const float4 s) {
    const float4 x = a, y = b;
    a.x = x.x * c.x - y.x * s.x; b.x = y.x * c.x + x.x * s.x;
    a.y = x.y * c.y - y.y * s.y; b.y = y.y * c.y + x.y * s.y;
    a.z = x.z * c.z - y.z * s.z; b.z = y.z * c.z + x.z * s.z;
    a.w = x.w * c.w - y.w * s.w; b.w = y.w * c.w + x.w * s.w;
}
__device__ __forceinline__ float4 neg4(const float4 v) { return make_float4(-v.x, -v.y, -v.z, -v.w); }

// 8 consecutive bf16 as two float4 through ONE 16-byte access
__device__ __forceinline__ void ld8(const bf16_t* p, float4& lo, float4& hi) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
    lo = make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]);
    hi = make_float4((float)t[4], (float)t[5], (float)t[6], (float)t[7]);
}
__device__ __forceinline__ void st8(bf16_t* p, const float4 lo, const float4 hi) {
    bf16x8 t;
    t[0] = (bf16_t)lo.x; t[1] = (bf16_t)lo.y; t[2] = (bf16_t)lo.z; t[3] = (bf16_t)lo.w;
    t[4] = (bf16_t)hi.x; t[5] = (bf16_t)hi.y; t[6] = (bf16_t)hi.z; t[7] = (bf16_t)hi.w;
    *reinterpret_cast<bf16x8*>(p) = t;
}

// One lane owns VEC columns i .. i + VEC of a head's first half AND the same columns of its second half, so a rotated pair never crosses
// lanes.  VEC = 8 (bf16, hd % 16 == 0) and VEC = 4 (fp32): 16-byte accesses; bf16 with hd % 16 == 8: VEC = 4, 8-byte accesses.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void rope_kernel(int rows, int H, int hd, T* __restrict__ x, int64_t ldx, const int32_t* __restrict__ pos,
                                                   const float* __restrict__ cosT, const float* __restrict__ sinT, int64_t ldt, int n_pos,
                                                   int inverse) {
    const int half = hd >> 1, per_head = half / VEC;
    const int64_t per_row = (int64_t)H * per_head, n = (int64_t)rows * per_row;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = idx / per_row;
        const int rem = (int)(idx - r * per_row), h = rem / per_head, i = (rem - h * per_head) * VEC;
        const int p = pos[r];
        if (p < 0 || p >= n_pos) continue;                        // out of range: the row stays as it is
        T* lo = x + r * ldx + (int64_t)h * hd + i;
        T* hi = lo + half;
        const float* cp = cosT + (int64_t)p * ldt + i;
        const float* sp = sinT + (int64_t)p * ldt + i;
        float4 c0 = *reinterpret_cast<const float4*>(cp), s0 = *reinterpret_cast<const float4*>(sp);
        if (inverse) s0 = neg4(s0);
        if constexpr (VEC == 8) {
            float4 c1 = *reinterpret_cast<const float4*>(cp + 4), s1 = *reinterpret_cast<const float4*>(sp + 4);
            if (inverse) s1 = neg4(s1);
            float4 a0, a1, b0, b1;
            ld8(lo, a0, a1);
            ld8(hi, b0, b1);
            rotate4(a0, b0, c0, s0);
            rotate4(a1, b1, c1, s1);
            st8(lo, a0, a1);
            st8(hi, b0, b1);
        } else {
            float4 a = elem<T>::ld4(lo), b = elem<T>::ld4(hi);
            rotate4(a, b, c0, s0);
            elem<T>::st4(lo, a);
            elem<T>::st4(hi, b);
        }
    }
}

__device__ __forceinline__ float4 sum_slices(const float* __restrict__ p, int64_t slice, int ks) {
    float4 v = *reinterpret_cast<const float4*>(p);
    for (int s = 1; s < ks; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(p + s * slice);
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    return v;
}

// Row m of [ks][M][3E] partial sums -> q | k | v in `T`.  A row has 2 H (hd / 8) rotated items (4 columns of each half of a q or k head)
// followed by E / 4 plain items (v).
template <typename T>
__global__ __launch_bounds__(256) void rope_finish_kernel(int M, int H, int hd, const float* __restrict__ P, int ks, const int32_t* __restrict__ pos,
                                                          const float* __restrict__ cosT, const float* __restrict__ sinT, int64_t ldt, int n_pos,
                                                          T* __restrict__ out, int64_t ldo) {
    const int E = H * hd, half = hd >> 1, per_head = half >> 2, n_rot = 2 * H * per_head, per_row = n_rot + (E >> 2);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * per_row) return;
    const int m = idx / per_row, it = idx - m * per_row;
    const int64_t N3 = 3 * (int64_t)E, slice = (int64_t)M * N3;
    const float* row = P + m * N3;
    T* o = out + (int64_t)m * ldo;
    if (it >= n_rot) {
        const int c = 2 * E + (it - n_rot) * 4;
        elem<T>::st4(o + c, sum_slices(row + c, slice, ks));
        return;
    }
    const int h = it / per_head, i = (it - h * per_head) * 4, c = h * hd + i;      // h runs over the 2 H heads of q | k
    float4 a = sum_slices(row + c, slice, ks), b = sum_slices(row + c + half, slice, ks);
    const int p = pos[m];
    if (p >= 0 && p < n_pos)
        rotate4(a, b, *reinterpret_cast<const float4*>(cosT + (int64_t)p * ldt + i), *reinterpret_cast<const float4*>(sinT + (int64_t)p * ldt + i));
    elem<T>::st4(o + c, a);
    elem<T>::st4(o + c + half, b);
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(int rows, int F, const T* __restrict__ u, int64_t ldu, T* __restrict__ h, int64_t ldh) {
    const int64_t n4 = (int64_t)rows * (F >> 2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / (F >> 2);
        const int c = (int)(i - r * (F >> 2)) * 4;
        const float4 g = elem<T>::ld4(u + r * ldu + c), b = elem<T>::ld4(u + r * ldu + F + c);
        elem<T>::st4(h + r * ldh + c, make_float4(silu(g.x) * b.x, silu(g.y) * b.y, silu(g.z) * b.z, silu(g.w) * b.w));
    }
}
template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(int rows, int F, const T* __restrict__ u, int64_t ldu, const T* __restrict__ dh, int64_t lddh,
                                                         T* __restrict__ du, int64_t lddu) {
    const int64_t n4 = (int64_t)rows * (F >> 2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / (F >> 2);
        const int c = (int)(i - r * (F >> 2)) * 4;
        const float4 g = elem<T>::ld4(u + r * ldu + c), b = elem<T>::ld4(u + r * ldu + F + c), d = elem<T>::ld4(dh + r * lddh + c);
        elem<T>::st4(du + r * lddu + c, make_float4(d.x * b.x * silu_grad(g.x), d.y * b.y * silu_grad(g.y), d.z * b.z * silu_grad(g.z),
                                                    d.w * b.w * silu_grad(g.w)));
        elem<T>::st4(du + r * lddu + F + c, make_float4(d.x * silu(g.x), d.y * silu(g.y), d.z * silu(g.z), d.w * silu(g.w)));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_splitk_kernel(int M, int F, const float* __restrict__ P, int ks, T* __restrict__ out, int64_t ld) {
    const int nq = F >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * nq) return;
    const int m = idx / nq, n = (idx - m * nq) * 4;
    const int64_t N2 = 2 * (int64_t)F, slice = (int64_t)M * N2;
    const float4 g = sum_slices(P + m * N2 + n, slice, ks), w = sum_slices(P + m * N2 + F + n, slice, ks);
    elem<T>::st4(out + (int64_t)m * ld + n, make_float4(silu(g.x) * w.x, silu(g.y) * w.y, silu(g.z) * w.z, silu(g.w) * w.w));
}

inline int elementwise_blocks(int64_t items) { return (int)std::min<int64_t>((items + 255) / 256, 256 * 8); }

// cos / sin tables of eavqa_rope / eavqa_rope_finish
inline int check_table(int hd, const int32_t* pos, const float* cosT, const float* sinT, int64_t ldt, int n_pos) {
    if (!pos || !cosT || !sinT || n_pos <= 0) return EAVQA_E_ARG;
    if (hd <= 0 || hd % 8 || hd > 256 || ldt < hd / 2) return EAVQA_E_SHAPE;
    if (ldt % 4 || !eavqa_aligned16(cosT) || !eavqa_aligned16(sinT)) return EAVQA_E_ALIGN;
    return EAVQA_OK;
}

// base pointers of the SwiGLU entry points: the kernels move 4 elements of `dtype` per access (8 bytes bfloat16, 16 bytes float32)
inline bool aligned_as(int dtype, const void* p) { return (reinterpret_cast<uintptr_t>(p) & (dtype == EAVQA_BF16 ? 7u : 15u)) == 0; }
}  // namespace

extern "C" int eavqa_rope(int dtype, int rows, int H, int hd, void* x, int64_t ldx, const int32_t* pos, const float* cos, const float* sin,
                          int64_t ld_table, int n_pos, int inverse, void* stream) {
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (!x || rows <= 0 || H <= 0) return EAVQA_E_ARG;
    if (const int rc = check_table(hd, pos, cos, sin, ld_table, n_pos)) return rc;
    if (ldx < (int64_t)H * hd) return EAVQA_E_SHAPE;
    if (!eavqa_aligned16(x) || ldx % (dtype == EAVQA_BF16 ? 8 : 4)) return EAVQA_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int inv = inverse != 0;
    if (dtype == EAVQA_F32) {
        const int blocks = elementwise_blocks((int64_t)rows * H * (hd / 8));
        hipLaunchKernelGGL((rope_kernel<float, 4>), dim3(blocks), dim3(256), 0, s, rows, H, hd, reinterpret_cast<float*>(x), ldx, pos, cos, sin, ld_table,
                           n_pos, inv);
    } else if (hd % 16 == 0) {
        const int blocks = elementwise_blocks((int64_t)rows * H * (hd / 16));
        hipLaunchKernelGGL((rope_kernel<bf16_t, 8>), dim3(blocks), dim3(256), 0, s, rows, H, hd, reinterpret_cast<bf16_t*>(x), ldx, pos, cos, sin, ld_table,
                           n_pos, inv);
    } else {
        const int blocks = elementwise_blocks((int64_t)rows * H * (hd / 8));
        hipLaunchKernelGGL((rope_kernel<bf16_t, 4>), dim3(blocks), dim3(256), 0, s, rows, H, hd, reinterpret_cast<bf16_t*>(x), ldx, pos, cos, sin, ld_table,
                           n_pos, inv);
    }
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_rope_finish(int dtype, int M, int H, int hd, const float* partials, int ks, const int32_t* pos, const float* cos,
                                 const float* sin, int64_t ld_table, int n_pos, void* out, int64_t ld_out, void* stream) {
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (!partials || !out || M <= 0 || H <= 0 || ks <= 0) return EAVQA_E_ARG;
    if (const int rc = check_table(hd, pos, cos, sin, ld_table, n_pos)) return rc;
    if (ld_out < 3 * (int64_t)H * hd || (int64_t)M * 3 * H * hd > (int64_t)1 << 30) return EAVQA_E_SHAPE;
    if (!eavqa_aligned16(partials) || !eavqa_aligned16(out) || ld_out % 4) return EAVQA_E_ALIGN;
    const int per_row = 2 * H * (hd / 8) + H * hd / 4, threads = M * per_row;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_BF16)
        hipLaunchKernelGGL(rope_finish_kernel<bf16_t>, dim3((threads + 255) / 256), dim3(256), 0, s, M, H, hd, partials, ks, pos, cos, sin, ld_table, n_pos,
                           reinterpret_cast<bf16_t*>(out), ld_out);
    else
        hipLaunchKernelGGL(rope_finish_kernel<float>, dim3((threads + 255) / 256), dim3(256), 0, s, M, H, hd, partials, ks, pos, cos, sin, ld_table, n_pos,
                           reinterpret_cast<float*>(out), ld_out);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_swiglu_fwd(int dtype, int rows, int F, const void* u, int64_t ldu, void* h, int64_t ldh, void* stream) {
    if (!u || !h || rows <= 0 || F <= 0) return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (F % 4 || ldu % 4 || ldh % 4 || ldu < 2 * (int64_t)F || ldh < F) return EAVQA_E_SHAPE;
    if (!aligned_as(dtype, u) || !aligned_as(dtype, h)) return EAVQA_E_ALIGN;
    const int blocks = elementwise_blocks((int64_t)rows * (F / 4));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_F32)
        hipLaunchKernelGGL(swiglu_fwd_kernel<float>, dim3(blocks), dim3(256), 0, s, rows, F, reinterpret_cast<const float*>(u), ldu, reinterpret_cast<float*>(h), ldh);
    else if (dtype == EAVQA_BF16)
        hipLaunchKernelGGL(swiglu_fwd_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, rows, F, reinterpret_cast<const bf16_t*>(u), ldu, reinterpret_cast<bf16_t*>(h), ldh);
    else return EAVQA_E_DTYPE;
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_swiglu_bwd(int dtype, int rows, int F, const void* u, int64_t ldu, const void* dh, int64_t lddh, void* du, int64_t lddu,
                                void* stream) {
    if (!u || !dh || !du || rows <= 0 || F <= 0) return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (F % 4 || ldu % 4 || lddh % 4 || lddu % 4 || ldu < 2 * (int64_t)F || lddu < 2 * (int64_t)F || lddh < F) return EAVQA_E_SHAPE;
    if (!aligned_as(dtype, u) || !aligned_as(dtype, dh) || !aligned_as(dtype, du)) return EAVQA_E_ALIGN;
    const int blocks = elementwise_blocks((int64_t)rows * (F / 4));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_F32)
        hipLaunchKernelGGL(swiglu_bwd_kernel<float>, dim3(blocks), dim3(256), 0, s, rows, F, reinterpret_cast<const float*>(u), ldu,
                           reinterpret_cast<const float*>(dh), lddh, reinterpret_cast<float*>(du), lddu);
    else if (dtype == EAVQA_BF16)
        hipLaunchKernelGGL(swiglu_bwd_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, rows, F, reinterpret_cast<const bf16_t*>(u), ldu,
                           reinterpret_cast<const bf16_t*>(dh), lddh, reinterpret_cast<bf16_t*>(du), lddu);
    else return EAVQA_E_DTYPE;
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_swiglu_splitk(int dtype, int M, int F, const float* partials, int ks, void* out, int64_t ld, void* stream) {
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (!partials || !out || M <= 0 || F <= 0 || ks <= 0) return EAVQA_E_ARG;
    if (F % 4 || ld % 4 || ld < F || (int64_t)M * F > (int64_t)1 << 30) return EAVQA_E_SHAPE;
    if (!eavqa_aligned16(partials) || !aligned_as(dtype, out)) return EAVQA_E_ALIGN;
    const int threads = M * (F / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_BF16)
        hipLaunchKernelGGL(swiglu_splitk_kernel<bf16_t>, dim3((threads + 255) / 256), dim3(256), 0, s, M, F, partials, ks, reinterpret_cast<bf16_t*>(out), ld);
    else
        hipLaunchKernelGGL(swiglu_splitk_kernel<float>, dim3((threads + 255) / 256), dim3(256), 0, s, M, F, partials, ks, reinterpret_cast<float*>(out), ld);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
