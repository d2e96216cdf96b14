// The normalisation family: LayerNorm and T5's RMS norm, forward / backward / over split-K partial sums (eavqa_layernorm_* / eavqa_rmsnorm_*
// in include/eavqa.h).  Every entry point fills a NormCall (norm_params.h) and calls launch().
// HBM-bound.  Row-per-wave kernels (forward, backward): one wavefront (64 lanes) owns one row, the row lives in registers between the
// statistics passes, every global access is a 16-byte (fp32) or 8-byte (bf16) vector; one body per pass serves both kinds (CENTER).
// Algorithmic bytes per row: fwd = cols*(sizeof x + sizeof y); bwd = cols*(x + dy + dres + dx).
// Workgroup-per-row kernel (ln_splitk_kernel): the decode step's residual add + split-K finish + norm in one pass.
#include "common.h"
#include "norm_params.h"

namespace {

// kind: 0 = T, 1 = float32, 2 = bfloat16, 3 = half (wave-uniform)
template <typename T>
__device__ __forceinline__ float4 ldrow4(const void* base, int64_t off, int kind) {
    if (kind == 1) return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off);
    if (kind == 2) return elem<bf16_t>::ld4(reinterpret_cast<const bf16_t*>(base) + off);
    if (kind == 3) return elem<f16_t>::ld4(reinterpret_cast<const f16_t*>(base) + off);
    return elem<T>::ld4(reinterpret_cast<const T*>(base) + off);
}

__device__ __forceinline__ float4 ldvec4(const float* p, int c, float fill) {
    return p ? *reinterpret_cast<const float4*>(p + 4 * c) : make_float4(fill, fill, fill, fill);
}

// The e4m3 row rule (norm_params.h) on a row that one wave holds in registers (lane l: float4 l, l + 64, ...; entries beyond nv are zeros).
// (eavqa_layernorm_fwd_fp8 / _bwd_fp8: the quantiser fused into its row-complete producers.)
template <int NV>
__device__ __forceinline__ void quantize_row_e4m3(const float4 (&v)[NV], int nv, int lane, unsigned char* q, float* scale_out) {
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (lane + 64 * i < nv) amax = fmaxf(amax, amax4(v[i]));
    const float scale = e4m3_row_scale(wave_max(amax));
    const float inv = 1.f / scale;
    if (lane == 0) *scale_out = scale;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) *reinterpret_cast<int*>(q + 4 * c) = e4m3_pack4(v[i], inv);
    }
}

// a^2 + b^2 + c^2 + d^2 as the kernels have always rounded it: two products, two fused multiply-adds, one add.  Spelled out and with
// contraction off, because left to the compiler the fusion moved with the shape of the loop around it (rms_fwd_kernel from NV = 4 on).
__device__ __forceinline__ float sumsq4(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    return fmaf(a, a, b * b) + fmaf(c, c, d * d);
}

// y = (x - mean) * rstd * gamma + beta; RMS (T5LayerNorm, HF:models/t5/modeling_t5.py:50-72; CENTER = false): y = gamma * x * rsqrt(mean(x^2)
// + eps) - no mean subtraction, no bias.  The variance is the second of two passes over the registers, about the mean (RMS: about 0).
template <typename T, int NV, bool CENTER>
__device__ __forceinline__ void norm_fwd_row(const NormRow c) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= c.rows) return;
    const int nv = c.cols >> 2;
    float4 v[NV], gm[NV], bt[NV];
    // gamma / beta are fetched together with the row: one memory round trip instead of two dependent ones
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = lane + 64 * i;
        if (col < nv) {
            v[i] = ldrow4<T>(c.x, (int64_t)row * c.ldx + 4 * col, c.x_kind);
            gm[i] = ldvec4(c.gamma, col, 1.f);
            if constexpr (CENTER) bt[i] = ldvec4(c.beta, col, 0.f);
        } else {
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    float mu = 0.f;
    if constexpr (CENTER) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        mu = wave_sum(s) / (float)c.cols;
    }
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < nv) {
            q += sumsq4(v[i].x - mu, v[i].y - mu, v[i].z - mu, v[i].w - mu);
        }
    }
    const float rs = rsqrtf(wave_sum(q) / (float)c.cols + c.eps);
    if (lane == 0) {
        if (CENTER && c.mean) c.mean[row] = mu;
        if (c.rstd) c.rstd[row] = rs;
    }
    T* y = reinterpret_cast<T*>(c.y);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = lane + 64 * i;
        if (col < nv) {
            float4 o = make_float4((v[i].x - mu) * rs * gm[i].x, (v[i].y - mu) * rs * gm[i].y, (v[i].z - mu) * rs * gm[i].z, (v[i].w - mu) * rs * gm[i].w);
            if constexpr (CENTER) { o.x += bt[i].x; o.y += bt[i].y; o.z += bt[i].z; o.w += bt[i].w; }
            if (y) elem<T>::st4(y + (int64_t)row * c.ldy + 4 * col, o);
            if (c.q) v[i] = round_to<T>(o);           // what eavqa_quantize_rows_fp8 would read back: the values in the storage type
        }
    }
    if (c.q) quantize_row_e4m3<NV>(v, nv, lane, c.q + (int64_t)row * c.ldq, c.q_scale + row);
}

// dx = dres + rstd * (g*dy - mean(g*dy) - xhat * mean(g*dy*xhat)); RMS (frozen weight): dx = dres + rstd * (g - xhat * mean(g * xhat)),
// g = w * dy, xhat = x * rstd
template <typename T, int NV, bool CENTER>
__device__ __forceinline__ void norm_bwd_row(const NormRow c) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= c.rows) return;
    const int nv = c.cols >> 2;
    float mu = 0.f;
    if constexpr (CENTER) mu = c.mean[row];
    const float rs = c.rstd[row];
    const T* dy = reinterpret_cast<const T*>(c.dy);
    T* dx_lowp = reinterpret_cast<T*>(c.dx_lowp);
    float4 xh[NV], gd[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = lane + 64 * i;
        if (col < nv) {
            const float4 xv = ldrow4<T>(c.x, (int64_t)row * c.ldx + 4 * col, c.x_kind);
            const float4 d = elem<T>::ld4(dy + (int64_t)row * c.lddy + 4 * col);
            const float4 g = ldvec4(c.gamma, col, 1.f);
            xh[i] = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
            gd[i] = make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w);
            if constexpr (CENTER) s1 += (gd[i].x + gd[i].y) + (gd[i].z + gd[i].w);
            s2 += (gd[i].x * xh[i].x + gd[i].y * xh[i].y) + (gd[i].z * xh[i].z + gd[i].w * xh[i].w);
        } else {
            xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            gd[i] = xh[i];
        }
    }
    float m1 = 0.f;
    if constexpr (CENTER) m1 = wave_sum(s1) / (float)c.cols;
    const float m2 = wave_sum(s2) / (float)c.cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = lane + 64 * i;
        if (col < nv) {
            const float4 r = c.dres ? *reinterpret_cast<const float4*>(c.dres + (int64_t)row * c.lddx + 4 * col) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 o;
            o.x = r.x + rs * (gd[i].x - m1 - xh[i].x * m2);
            o.y = r.y + rs * (gd[i].y - m1 - xh[i].y * m2);
            o.z = r.z + rs * (gd[i].z - m1 - xh[i].z * m2);
            o.w = r.w + rs * (gd[i].w - m1 - xh[i].w * m2);
            *reinterpret_cast<float4*>(c.dx + (int64_t)row * c.lddx + 4 * col) = o;
            if (dx_lowp) elem<T>::st4(dx_lowp + (int64_t)row * c.ld_lowp + 4 * col, o);
            if (c.q) gd[i] = round_to<T>(o);          // (gd is dead from here on)
        }
    }
    if (c.q) quantize_row_e4m3<NV>(gd, nv, lane, c.q + (int64_t)row * c.ldq, c.q_scale + row);
}

// The four row kernels, under the names profiles/ and bench.py's HBM table join on (the RMS forms keep names of their own).  They take
// NormRow's fields as plain arguments, in the order these kernels have always had: a struct as the kernel argument, and another order of
// the plain ones, both measured slower per launch on the MI355X (profiles/norm_one_host_layer.md).  No entry point asks for RMS rows as
// e4m3, so those two leave q null and the quantiser folds away (it would cost the bf16 backward ten registers and an occupancy step).
template <typename T, int NV>
__global__ __launch_bounds__(256) void ln_fwd_kernel(int x_kind, int rows, int cols, const void* x, int64_t ldx, const float* gamma,
                                                     const float* beta, float eps, void* y, int64_t ldy, float* mean, float* rstd,
                                                     unsigned char* q, int64_t ldq, float* q_scale) {
    norm_fwd_row<T, NV, true>(NormRow{x_kind, rows, cols, x, ldx, gamma, beta, eps, y, ldy, mean, rstd, q, ldq, q_scale});
}
template <typename T, int NV>
__global__ __launch_bounds__(256) void rms_fwd_kernel(int x_kind, int rows, int cols, const void* x, int64_t ldx, const float* gamma, const float*,
                                                      float eps, void* y, int64_t ldy, float*, float* rstd, unsigned char*, int64_t, float*) {
    norm_fwd_row<T, NV, false>(NormRow{x_kind, rows, cols, x, ldx, gamma, nullptr, eps, y, ldy, nullptr, rstd});
}
template <typename T, int NV>
__global__ __launch_bounds__(256) void ln_bwd_kernel(int x_kind, int rows, int cols, const void* x, int64_t ldx, const void* dy, int64_t lddy,
                                                     const float* gamma, float* mean, float* rstd, const float* dres, float* dx, int64_t lddx,
                                                     void* dx_lowp, int64_t ld_lowp, unsigned char* q, int64_t ldq, float* q_scale) {
    norm_bwd_row<T, NV, true>(NormRow{x_kind, rows, cols, x, ldx, gamma, nullptr, 0.f, nullptr, 0, mean, rstd, q, ldq, q_scale, dy, lddy, dres, dx,
                                      lddx, dx_lowp, ld_lowp});
}
template <typename T, int NV>
__global__ __launch_bounds__(256) void rms_bwd_kernel(int x_kind, int rows, int cols, const void* x, int64_t ldx, const void* dy, int64_t lddy,
                                                      const float* gamma, float*, float* rstd, const float* dres, float* dx, int64_t lddx,
                                                      void* dx_lowp, int64_t ld_lowp, unsigned char*, int64_t, float*) {
    norm_bwd_row<T, NV, false>(NormRow{x_kind, rows, cols, x, ldx, gamma, nullptr, 0.f, nullptr, 0, nullptr, rstd, nullptr, 0, nullptr, dy, lddy,
                                       dres, dx, lddx, dx_lowp, ld_lowp});
}

// dgamma[c] += sum_r dy[r,c] * xhat[r,c], dbeta[c] += sum_r dy[r,c] (the mapper's LayerNorms only: the LM is frozen).  A block owns 64
// columns x 64 rows, sums them in registers / LDS and issues ONE atomic per column: rows / 64 atomics per column instead of one per
// element (2 048 x 4 096 elements cost 440-540 us through the atomic units, MI355X_MICROARCH.md "Global float atomics").
template <typename T>
__global__ __launch_bounds__(256) void ln_dparam_kernel(int x_f32, int rows, int cols, const void* x, int64_t ldx, const T* dy, int64_t lddy,
                                                        const float* mean, const float* rstd, float* dgamma, float* dbeta) {
    __shared__ float sg[4][64], sb[4][64];
    const int tid = threadIdx.x, cl = tid & 63, rs = tid >> 6;
    const int col = blockIdx.x * 64 + cl;
    float g = 0.f, b = 0.f;
    if (col < cols) {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int row = blockIdx.y * 64 + rs + 4 * i;
            if (row < rows) {
                const int64_t off = (int64_t)row * ldx + col;
                const float xv = x_f32 ? reinterpret_cast<const float*>(x)[off] : elem<T>::ld(reinterpret_cast<const T*>(x) + off);
                const float d = elem<T>::ld(dy + (int64_t)row * lddy + col);
                g += d * (xv - mean[row]) * rstd[row];
                b += d;
            }
        }
    }
    sg[rs][cl] = g; sb[rs][cl] = b;
    __syncthreads();
    if (tid < 64 && col < cols) {
        if (dgamma) atomicAdd(dgamma + col, (sg[0][cl] + sg[1][cl]) + (sg[2][cl] + sg[3][cl]));
        if (dbeta) atomicAdd(dbeta + col, (sb[0][cl] + sb[1][cl]) + (sb[2][cl] + sb[3][cl]));
    }
}

// one 512-thread workgroup per row (a decode step has at most 64 rows: parallelism must come from inside the row), the
// partial-sum loads of eight slices in flight at once: x = x_in + bias + sum_s P[s]; y = LN(x) * gamma + beta
// NV float4 per thread: rows of up to 2048 NV columns; NV = 8 (rows of up to LNS_MAX_COLS = 16384 columns) keeps two slices in flight
// instead of eight: the row, gamma and beta alone are 96 registers (the output row comes on top), and eight slices would be 256 more.  Two
// is chosen to fit the register file, not measured: no product path has rows that wide yet (nor the NV = 4 form's 4096..8192 columns).
// The slices are added in index order whatever the batch, so the sum is the same.
__device__ __forceinline__ float block_sum8(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
}

template <typename T, int NV>
__global__ __launch_bounds__(LNS_NT) void ln_splitk_kernel(int rows, int cols, const float* __restrict__ x_in, int64_t ldx,
                                                           const float* __restrict__ P, int ks, const float* __restrict__ bias,
                                                           float* __restrict__ x_out, int64_t ldxo, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, T* __restrict__ y, int64_t ldy, int rms,
                                                           unsigned char* __restrict__ yq, int64_t ldq, float* __restrict__ yq_scale) {
    __shared__ float red[LNS_NT / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int nv = cols >> 2;
    float4 v[NV], gm[NV], bt[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = tid + LNS_NT * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < nv) {
            v[i] = *reinterpret_cast<const float4*>(x_in + (int64_t)row * ldx + 4 * c);
            gm[i] = *reinterpret_cast<const float4*>(gamma + 4 * c);
            bt[i] = rms ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(beta + 4 * c);
            if (bias) { const float4 b = *reinterpret_cast<const float4*>(bias + 4 * c); v[i].x += b.x; v[i].y += b.y; v[i].z += b.z; v[i].w += b.w; }
        }
    }
    const int64_t slice = (int64_t)rows * cols;
    const float* prow = P + (int64_t)row * cols;
    constexpr int UB = NV <= 4 ? 8 : 2;           // slices in flight
    int sl = 0;
    for (; sl + UB <= ks; sl += UB) {
        float4 t[UB][NV];
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = tid + LNS_NT * i;
                t[u][i] = c < nv ? *reinterpret_cast<const float4*>(prow + (sl + u) * slice + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
        for (int u = 0; u < UB; ++u)         // slices are added in index order: the sum does not depend on scheduling
#pragma unroll
            for (int i = 0; i < NV; ++i) { v[i].x += t[u][i].x; v[i].y += t[u][i].y; v[i].z += t[u][i].z; v[i].w += t[u][i].w; }
    }
    if (sl < ks) {
        float4 t[UB][NV];
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = tid + LNS_NT * i;
                t[u][i] = (c < nv && sl + u < ks) ? *reinterpret_cast<const float4*>(prow + (sl + u) * slice + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (sl + u < ks) { v[i].x += t[u][i].x; v[i].y += t[u][i].y; v[i].z += t[u][i].z; v[i].w += t[u][i].w; }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = tid + LNS_NT * i;
        if (c < nv) {
            if (x_out) *reinterpret_cast<float4*>(x_out + (int64_t)row * ldxo + 4 * c) = v[i];
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    // rms (T5LayerNorm, HF:t5 :50-72): no mean subtraction, no bias - y = gamma * x * rsqrt(mean(x^2) + eps)
    const float mu = rms ? 0.f : block_sum8(s, red) / (float)cols;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = tid + LNS_NT * i;
        if (c < nv) {
            const float a = v[i].x - mu, b = v[i].y - mu, cc = v[i].z - mu, d = v[i].w - mu;
            q += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rs = rsqrtf(block_sum8(q, red) / (float)cols + eps);
    float4 o[NV];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = tid + LNS_NT * i;
        if (c < nv) {
            o[i].x = (v[i].x - mu) * rs * gm[i].x + bt[i].x;
            o[i].y = (v[i].y - mu) * rs * gm[i].y + bt[i].y;
            o[i].z = (v[i].z - mu) * rs * gm[i].z + bt[i].z;
            o[i].w = (v[i].w - mu) * rs * gm[i].w + bt[i].w;
            if (y) elem<T>::st4(y + (int64_t)row * ldy + 4 * c, o[i]);
            if (yq) {          // what eavqa_quantize_rows_fp8 would see: the values rounded to the storage type first
                o[i] = round_to<T>(o[i]);
                amax = fmaxf(amax, amax4(o[i]));
            }
        }
    }
    if (yq) {
        // the e4m3 row rule (norm_params.h), the row's amax reduced over the eight waves through LDS
        amax = wave_max(amax);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = amax;
        __syncthreads();
        amax = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
        const float scale = e4m3_row_scale(amax);
        const float inv = 1.f / scale;
        if (tid == 0) yq_scale[row] = scale;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = tid + LNS_NT * i;
            if (c < nv) *reinterpret_cast<int*>(yq + (int64_t)row * ldq + 4 * c) = e4m3_pack4(o[i], inv);
        }
    }
}

// One launcher: the storage type picks the instantiation, the row width its float4 count per thread.
template <typename T> int launch_as(const NormCall& c) {
    constexpr bool half = std::is_same_v<T, f16_t>;          // LayerNorm forward's alone (validate): nothing else is instantiated for it
    const bool layer = c.kind == NORM_LAYER;
    const int nv = (c.cols / 4 + 63) / 64;
    const dim3 grid((c.rows + LN_WAVES - 1) / LN_WAVES), block(256);
    if (c.pass == NORM_FWD) {
        with_nv<2, LN_MAX_V4>(nv, [&](auto n) {
            constexpr int NV = decltype(n)::value;
            auto kernel = ln_fwd_kernel<T, NV>;
            if constexpr (!half) kernel = layer ? kernel : rms_fwd_kernel<T, NV>;
            hipLaunchKernelGGL(kernel, grid, block, 0, c.stream, c.x_kind, c.rows, c.cols, c.x, c.ldx, c.gamma, c.beta, c.eps, c.y, c.ldy, c.mean,
                               c.rstd, c.q, c.ldq, c.q_scale);
        });
    } else if constexpr (!half) {
        if (c.pass == NORM_BWD) {
            with_nv<2, LN_MAX_V4_BWD>(nv, [&](auto n) {
                constexpr int NV = decltype(n)::value;
                hipLaunchKernelGGL((layer ? ln_bwd_kernel<T, NV> : rms_bwd_kernel<T, NV>), grid, block, 0, c.stream, c.x_kind, c.rows, c.cols, c.x,
                                   c.ldx, c.dy, c.lddy, c.gamma, c.mean, c.rstd, c.dres, c.dx, c.lddx, c.dx_lowp, c.ld_lowp, c.q, c.ldq, c.q_scale);
            });
            if (c.dgamma || c.dbeta)
                hipLaunchKernelGGL((ln_dparam_kernel<T>), dim3((c.cols + 63) / 64, (c.rows + 63) / 64), dim3(256), 0, c.stream, c.x_kind, c.rows,
                                   c.cols, c.x, c.ldx, reinterpret_cast<const T*>(c.dy), c.lddy, c.mean, c.rstd, c.dgamma, c.dbeta);
        } else {
            with_nv<1, LNS_MAX_V4>((c.cols / 4 + LNS_NT - 1) / LNS_NT, [&](auto n) {
                hipLaunchKernelGGL((ln_splitk_kernel<T, decltype(n)::value>), dim3(c.rows), dim3(LNS_NT), 0, c.stream, c.rows, c.cols,
                                   reinterpret_cast<const float*>(c.x), c.ldx, c.partials, c.ks, c.bias, c.x_out, c.ld_out, c.gamma, c.beta, c.eps,
                                   reinterpret_cast<T*>(c.y), c.ldy, (int)(c.kind == NORM_RMS), c.q, c.ldq, c.q_scale);
            });
        }
    }
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

int launch(NormCall c, void* stream) {
    if (const int rc = validate(c)) return rc;
    c.stream = reinterpret_cast<hipStream_t>(stream);
    if (c.pass != NORM_SPLITK && c.dtype == EAVQA_F32 && c.x_kind == 0) c.x_kind = 1;      // (SPLITK: x is float32 whatever the storage type)
    return c.dtype == EAVQA_F32 ? launch_as<float>(c) : c.dtype == EAVQA_BF16 ? launch_as<bf16_t>(c) : launch_as<f16_t>(c);
}

}  // namespace

extern "C" int eavqa_layernorm_fwd(int dtype, int x_kind, int rows, int cols, const void* x, int64_t ldx,
                                   const float* gamma, const float* beta, float eps, void* y, int64_t ldy,
                                   float* mean, float* rstd, void* stream) {
    NormCall c;
    c.dtype = dtype; c.x_kind = x_kind; c.rows = rows; c.cols = cols; c.x = x; c.ldx = ldx;
    c.gamma = gamma; c.beta = beta; c.eps = eps; c.y = y; c.ldy = ldy; c.mean = mean; c.rstd = rstd;
    return launch(c, stream);
}

extern "C" int eavqa_layernorm_fwd_fp8(int x_kind, int rows, int cols, const void* x, int64_t ldx, const float* gamma, const float* beta,
                                       float eps, void* yq, int64_t ldq, float* row_scale, float* mean, float* rstd, void* stream) {
    NormCall c;
    c.fp8 = true; c.x_kind = x_kind; c.rows = rows; c.cols = cols; c.x = x; c.ldx = ldx;
    c.gamma = gamma; c.beta = beta; c.eps = eps; c.mean = mean; c.rstd = rstd;
    c.q = reinterpret_cast<unsigned char*>(yq); c.ldq = ldq; c.q_scale = row_scale;
    return launch(c, stream);
}

namespace {
// what the four backward entry points share (mean: LayerNorm's only)
NormCall bwd_call(int kind, int dtype, int x_kind, int rows, int cols, const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* gamma,
                  const float* mean, const float* rstd, const float* dres, float* dx, int64_t lddx) {
    NormCall c;
    c.kind = kind; c.pass = NORM_BWD; c.dtype = dtype; c.x_kind = x_kind; c.rows = rows; c.cols = cols; c.x = x; c.ldx = ldx;
    c.dy = dy; c.lddy = lddy; c.gamma = gamma; c.mean = const_cast<float*>(mean); c.rstd = const_cast<float*>(rstd);
    c.dres = dres; c.dx = dx; c.lddx = lddx;
    return c;
}
}  // namespace

// x_f32 is x_kind restricted to 0 / 1 (validate); with float32 storage it has never been looked at
extern "C" int eavqa_layernorm_bwd(int dtype, int x_f32, int rows, int cols, const void* x, int64_t ldx,
                                   const void* dy, int64_t lddy, const float* gamma, const float* mean,
                                   const float* rstd, const float* dres, float* dx, int64_t lddx,
                                   float* dgamma, float* dbeta, void* dx_lowp, int64_t ld_lowp, void* stream) {
    NormCall c = bwd_call(NORM_LAYER, dtype, dtype == EAVQA_F32 ? 1 : x_f32, rows, cols, x, ldx, dy, lddy, gamma, mean, rstd, dres, dx, lddx);
    c.dgamma = dgamma; c.dbeta = dbeta; c.dx_lowp = dx_lowp; c.ld_lowp = ld_lowp;
    return launch(c, stream);
}

extern "C" int eavqa_layernorm_bwd_fp8(int x_f32, int rows, int cols, const void* x, int64_t ldx, const void* dy, int64_t lddy,
                                       const float* gamma, const float* mean, const float* rstd, const float* dres, float* dx, int64_t lddx,
                                       void* dxq, int64_t ldq, float* row_scale, void* stream) {
    NormCall c = bwd_call(NORM_LAYER, EAVQA_BF16, x_f32, rows, cols, x, ldx, dy, lddy, gamma, mean, rstd, dres, dx, lddx);
    c.fp8 = true; c.q = reinterpret_cast<unsigned char*>(dxq); c.ldq = ldq; c.q_scale = row_scale;
    return launch(c, stream);
}

extern "C" int eavqa_rmsnorm_fwd(int dtype, int x_kind, int rows, int cols, const void* x, int64_t ldx, const float* gamma, float eps,
                                 void* y, int64_t ldy, float* rstd, void* stream) {
    NormCall c;
    c.kind = NORM_RMS; c.dtype = dtype; c.x_kind = x_kind; c.rows = rows; c.cols = cols; c.x = x; c.ldx = ldx;
    c.gamma = gamma; c.eps = eps; c.y = y; c.ldy = ldy; c.rstd = rstd;
    return launch(c, stream);
}

extern "C" int eavqa_rmsnorm_bwd(int dtype, int x_kind, int rows, int cols, const void* x, int64_t ldx, const void* dy, int64_t lddy,
                                 const float* gamma, const float* rstd, const float* dres, float* dx, int64_t lddx, void* dx_lowp,
                                 int64_t ld_lowp, void* stream) {
    NormCall c = bwd_call(NORM_RMS, dtype, x_kind, rows, cols, x, ldx, dy, lddy, gamma, nullptr, rstd, dres, dx, lddx);
    c.dx_lowp = dx_lowp; c.ld_lowp = ld_lowp;
    return launch(c, stream);
}

namespace {
// what the three split-K entry points share
NormCall splitk_call(int kind, int dtype, int rows, int cols, const float* x_in, int64_t ldx, const float* partials, int ks, const float* bias,
                     float* x_out, int64_t ld_out, const float* gamma, const float* beta, float eps) {
    NormCall c;
    c.kind = kind; c.pass = NORM_SPLITK; c.dtype = dtype; c.rows = rows; c.cols = cols; c.x = x_in; c.ldx = ldx;
    c.partials = partials; c.ks = ks; c.bias = bias; c.x_out = x_out; c.ld_out = ld_out; c.gamma = gamma; c.beta = beta; c.eps = eps;
    return c;
}
}  // namespace

extern "C" int eavqa_layernorm_splitk(int dtype, int rows, int cols, const float* x_in, int64_t ldx, const float* partials, int ks,
                                      const float* bias, float* x_out, int64_t ld_out, const float* gamma, const float* beta,
                                      float eps, void* y, int64_t ldy, void* stream) {
    NormCall c = splitk_call(NORM_LAYER, dtype, rows, cols, x_in, ldx, partials, ks, bias, x_out, ld_out, gamma, beta, eps);
    c.y = y; c.ldy = ldy;
    return launch(c, stream);
}

extern "C" int eavqa_layernorm_splitk_fp8(int rows, int cols, const float* x_in, int64_t ldx, const float* partials, int ks, const float* bias,
                                          float* x_out, int64_t ld_out, const float* gamma, const float* beta, float eps, void* yq, int64_t ldq,
                                          float* row_scale, void* stream) {
    NormCall c = splitk_call(NORM_LAYER, EAVQA_BF16, rows, cols, x_in, ldx, partials, ks, bias, x_out, ld_out, gamma, beta, eps);
    c.q = reinterpret_cast<unsigned char*>(yq); c.ldq = ldq; c.q_scale = row_scale;
    return launch(c, stream);
}

extern "C" int eavqa_rmsnorm_splitk(int dtype, int rows, int cols, const float* x_in, int64_t ldx, const float* partials, int ks,
                                    float* x_out, int64_t ld_out, const float* gamma, float eps, void* y, int64_t ldy, void* stream) {
    NormCall c = splitk_call(NORM_RMS, dtype, rows, cols, x_in, ldx, partials, ks, nullptr, x_out, ld_out, gamma, nullptr, eps);
    c.y = y; c.ldy = ldy;
    return launch(c, stream);
}
