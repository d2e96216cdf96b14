// Decode-step kernels (one new token per sample, M = batch <= 64 rows): the step is a weight-streaming problem, HBM bound
// on the 12 E^2 weights of every layer, and a chain of short dependent kernels.  Two pieces here (eavqa.h):
//
//   eavqa_gemm_splitk      P[s][m][n] = sum_{k in slice s} A[m,k] B[n,k]        (bf16 in, fp32 partial sums out)
//   eavqa_splitk_finish    out = act(sum_s P[s] + bias) (+ residual), columns cut into up to 3 destination segments
//                          (q | k-cache row | v-cache row: the K/V append is the finish of the QKV projection)
//
// The third consumer of the partial sums, eavqa_layernorm_splitk (residual add + finish + norm in one pass), lives with the other
// normalisation kernels in norm.hip.
//
// Why split K over workgroups: with M <= 64 every workgroup needs the whole activation slab A, and the first skinny
// kernel (16 columns x all of K per workgroup) pulled 2 bytes of A through the CU's L1 for every byte of weights: the
// L2 -> CU path (about 55 GB/s per CU), not HBM, set its 2.4 TB/s.  Here a workgroup owns 128 columns x one K slice: its
// A slice is staged ONCE in LDS (LDS-DMA, swizzled 64-byte rows as in the tiled GEMMs) and shared by the eight waves, each
// of which streams its own 16 weight rows straight into VGPRs through a rolling window of 8 / 16 loads in flight.  A-bytes
// per weight byte: 16 MF / 128 = 0.25 (MF = 2).  The partial sums (ks x M x N fp32, 5-20 % of the weight bytes) are summed
// in a fixed order by the consumer, so the result does not depend on scheduling.  A pure-load kernel with the same access
// pattern reads these matrices at 4.3-4.7 TB/s (tools/hbm_probe.hip; 5.7 TB/s for 250+ MB): that is the floor this kernel is
// measured against, not 8 TB/s.
#include "decode_params.h"

namespace {

__device__ __forceinline__ int fswz(int row, int kc) { return row * 64 + ((kc ^ ((-(row >> 2)) & 3)) << 4); }


// MF: 16-row fragments of A (M <= 16 MF); NF: 16-column fragments per wave; NW: waves per workgroup (columns per workgroup =
// 16 NF NW: the A slice is staged once per workgroup, so A bytes per weight byte = 16 MF / (16 NF NW)); U: k-steps of weight loads in
// flight per wave.
template <int MF, int NF, int NW, int U>
__global__ __launch_bounds__(64 * NW) void gemm_bf16_splitk_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                   const bf16_t* __restrict__ B, int64_t ldb,
                                                                   float* __restrict__ P, int M, int N, int KS) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TILE = 16 * MF * 64;                      // bytes of one [16 MF rows][32 k] A tile
    constexpr int COLS = 16 * NF * NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * COLS + wave * 16 * NF, slice = blockIdx.y, k0 = slice * KS;
    const int nsteps = KS >> 5;

    // ---- this wave's 16 NF weight rows: the first U k-steps go out before anything else (they are the HBM round trip that
    //      bounds the workgroup's life; the A slice below comes from L2)
    const int x = lane & 15, g = lane >> 4;
    const bf16_t* bp[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) bp[j] = B + (int64_t)min(n0 + 16 * j + x, N - 1) * ldb + k0 + 8 * g;
    bf16x8 bf[U][NF];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < NF; ++j) bf[u][j] = *reinterpret_cast<const bf16x8*>(bp[j] + 32 * min(u, nsteps - 1));

    // ---- stage the A slice: chunk c -> tile c / (64 MF), row (c % (64 MF)) >> 2, physical slot c & 3
    const int total = nsteps * 64 * MF;
    for (int base = wave * 64; base < total; base += 64 * NW) {
        const int c = base + lane;
        if (c < total) {
            const int t = c / (64 * MF), within = c % (64 * MF);
            const int row = within >> 2, pc = within & 3;
            const bf16_t* src = A + (int64_t)min(row, M - 1) * lda + k0 + t * 32 + ((pc ^ ((-(row >> 2)) & 3)) << 3);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(smem + base * 16), 16, 0, 0);
        }
    }
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int a_off = fswz(x, g);
    __builtin_amdgcn_s_waitcnt(0x0070 | 0x0F00);     // vmcnt(0): A slice (and the first weights) have landed
    __syncthreads();

    // rolling window: the registers of k-step s are refilled with k-step s + U as soon as its MFMAs are issued, so U loads
    // per fragment column stay in flight for the whole slice
    for (int s0 = 0; s0 < nsteps; s0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bf16x8 w[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) w[j] = bf[u][j];
            if (s0 + U + u < nsteps) {
#pragma unroll
                for (int j = 0; j < NF; ++j) bf[u][j] = *reinterpret_cast<const bf16x8*>(bp[j] + 32 * (s0 + U + u));
            }
            if (s0 + u < nsteps) {
                const char* tile = smem + (s0 + u) * TILE;
#pragma unroll
                for (int i = 0; i < MF; ++i) {
                    const bf16x8 af = *reinterpret_cast<const bf16x8*>(tile + a_off + i * 1024);
#pragma unroll
                    for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, w[j], acc[i][j], 0, 0, 0);
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + 16 * j + x;
        if (n < N) {
            float* out = P + (int64_t)slice * M * N + n;
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 16 * i + 4 * g + r;
                    if (m < M) out[(int64_t)m * N] = acc[i][j][r];
                }
        }
    }
}

// The same kernel for a frozen LM held in e4m3 (BASELINE configs[4]): A = the activation rows quantised to e4m3 with one scale per row
// (eavqa_quantize_rows_fp8 / the fp8 output of eavqa_layernorm_splitk), B = e4m3 weights with one scale per tensor.  A k-step is 128 values
// = one whole 128-byte line per row and ONE v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales - the instruction eavqa_gemm_fp8 uses,
// so the partial sums differ from its accumulator by fp32 summation order only (the plain v_mfma_f32_16x16x32_fp8_fp8 adds its products with
// fewer guard bits: 2e-5 relative against float64 - enough, through the e4m3 rounding of every following activation, to move logits by
// percents between the cached and the re-forward generation).  Lane (x, g) holds the 16-byte chunks g and g + 4 of its row's step for both
// operands (gemm_fp8.hip's fragment layout).  The row and tensor scales are applied before the partial sums are written: every consumer of
// bf16 partial sums (LayerNorm pass, finish, decode attention) takes them unchanged.  Half the weight bytes per step of the bf16 decode.
typedef __attribute__((ext_vector_type(8))) int dec_i32x8;
template <int MF, int NF, int NW, int U>
__global__ __launch_bounds__(64 * NW) void gemm_fp8_splitk_kernel(const unsigned char* __restrict__ A, int64_t lda, const float* __restrict__ a_scale,
                                                                  const unsigned char* __restrict__ B, int64_t ldb, float b_scale,
                                                                  float* __restrict__ P, int M, int N, int KS) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TILE = 16 * MF * 128;                     // bytes of one [16 MF rows][128 k] A tile
    constexpr int COLS = 16 * NF * NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * COLS + wave * 16 * NF, slice = blockIdx.y, k0 = slice * KS;
    const int nsteps = KS >> 7;
    const int x = lane & 15, g = lane >> 4;
    const unsigned char* bp[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) bp[j] = B + (int64_t)min(n0 + 16 * j + x, N - 1) * ldb + k0 + 16 * g;
    uint4 blo[U][NF], bhi[U][NF];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            blo[u][j] = *reinterpret_cast<const uint4*>(bp[j] + 128 * min(u, nsteps - 1));
            bhi[u][j] = *reinterpret_cast<const uint4*>(bp[j] + 128 * min(u, nsteps - 1) + 64);
        }
    // A slice: chunk c -> tile c / (128 MF), row (c % (128 MF)) >> 3, physical slot c & 7 holds logical chunk slot ^ (row & 7)
    const int total = nsteps * 128 * MF;
    for (int base = wave * 64; base < total; base += 64 * NW) {
        const int c = base + lane;
        if (c < total) {
            const int t = c / (128 * MF), within = c % (128 * MF);
            const int row = within >> 3, pc = within & 7;
            const unsigned char* src = A + (int64_t)min(row, M - 1) * lda + k0 + t * 128 + ((pc ^ (row & 7)) << 4);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(smem + base * 16), 16, 0, 0);
        }
    }
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int a_off = x * 128 + ((g ^ (x & 7)) << 4);       // chunk g; chunk g + 4 sits at a_off ^ 64
    __builtin_amdgcn_s_waitcnt(0x0070 | 0x0F00);
    __syncthreads();
    auto frag = [](const uint4& lo, const uint4& hi) {
        return (dec_i32x8){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    };
    for (int s0 = 0; s0 < nsteps; s0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            dec_i32x8 w[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) w[j] = frag(blo[u][j], bhi[u][j]);
            if (s0 + U + u < nsteps) {
#pragma unroll
                for (int j = 0; j < NF; ++j) {
                    blo[u][j] = *reinterpret_cast<const uint4*>(bp[j] + 128 * (s0 + U + u));
                    bhi[u][j] = *reinterpret_cast<const uint4*>(bp[j] + 128 * (s0 + U + u) + 64);
                }
            }
            if (s0 + u < nsteps) {
                const char* tile = smem + (s0 + u) * TILE;
#pragma unroll
                for (int i = 0; i < MF; ++i) {
                    const dec_i32x8 af = frag(*reinterpret_cast<const uint4*>(tile + a_off + i * 2048),
                                              *reinterpret_cast<const uint4*>(tile + (a_off ^ 64) + i * 2048));
#pragma unroll
                    for (int j = 0; j < NF; ++j)      // cbsz = blgp = 0: both operands e4m3; block scales 2^0 (E8M0 byte 127)
                        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, w[j], acc[i][j], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + 16 * j + x;
        if (n < N) {
            float* out = P + (int64_t)slice * M * N + n;
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 16 * i + 4 * g + r;
                    if (m < M) out[(int64_t)m * N] = acc[i][j][r] * (a_scale[m] * b_scale);
                }
        }
    }
}

// out[m, n] = act(sum_s P[s][m][n] + bias[n]) (+ residual[m, n]); 4 columns per thread
template <typename T>
__global__ __launch_bounds__(256) void splitk_finish_kernel(int M, int N, const float* __restrict__ P, int ks, const float* __restrict__ bias,
                                                            int act, const float* __restrict__ residual, int64_t ldr, int out_f32,
                                                            int seg_cols, FinishSeg s0, FinishSeg s1, FinishSeg s2) {
    const int nq = N >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * nq) return;
    const int m = idx / nq, n = (idx % nq) * 4;
    float4 v = *reinterpret_cast<const float4*>(P + (int64_t)m * N + n);
    for (int s = 1; s < ks; ++s) {
        const float4 t = *reinterpret_cast<const float4*>(P + ((int64_t)s * M + m) * N + n);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    if (bias) { const float4 b = *reinterpret_cast<const float4*>(bias + n); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
    v.x = act_fwd(act, v.x); v.y = act_fwd(act, v.y); v.z = act_fwd(act, v.z); v.w = act_fwd(act, v.w);
    if (residual) {
        const float4 r = *reinterpret_cast<const float4*>(residual + (int64_t)m * ldr + n);
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    const int seg = n / seg_cols, nl = n - seg * seg_cols;
    const FinishSeg d = seg == 0 ? s0 : (seg == 1 ? s1 : s2);
    if (out_f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(d.dst) + (int64_t)m * d.ld + nl) = v;
    else elem<T>::st4(reinterpret_cast<T*>(d.dst) + (int64_t)m * d.ld + nl, v);
}

// h[m, c] = act(sum_s P[s][m][c]) * sum_s P[s][m][F + c]: the finish of T5's [wi_0; wi_1] projection (HF:t5 :97-123); 4 columns per thread
template <typename T>
__global__ __launch_bounds__(256) void splitk_finish_gated_kernel(int M, int F, const float* __restrict__ P, int ks, int act, T* __restrict__ out,
                                                                  int64_t ld) {
    const int nq = F >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * nq) return;
    const int m = idx / nq, n = (idx % nq) * 4;
    const int64_t N2 = 2 * (int64_t)F;
    float4 u = *reinterpret_cast<const float4*>(P + m * N2 + n), w = *reinterpret_cast<const float4*>(P + m * N2 + F + n);
    for (int s = 1; s < ks; ++s) {
        const float* ps = P + ((int64_t)s * M + m) * N2 + n;
        const float4 a = *reinterpret_cast<const float4*>(ps), b = *reinterpret_cast<const float4*>(ps + F);
        u.x += a.x; u.y += a.y; u.z += a.z; u.w += a.w;
        w.x += b.x; w.y += b.y; w.z += b.z; w.w += b.w;
    }
    float4 v;
    v.x = act_fwd(act, u.x) * w.x; v.y = act_fwd(act, u.y) * w.y; v.z = act_fwd(act, u.z) * w.z; v.w = act_fwd(act, u.w) * w.w;
    elem<T>::st4(out + (int64_t)m * ld + n, v);
}

// f(kernel, is it an fp8 kernel) for the plan's variant: every instantiated split-K kernel is named here (decode_params.h: splitk_instantiated)
template <typename F> bool with_splitk_kernel(bool fp8, const SplitKPlan& p, F&& f) {
    return with_value<1, 2, 4>(p.mf, [&](auto MF) {
        if (fp8)
            return p.nf == 1 && p.nw == 8 &&
                   with_value<4, 8>(p.u, [&](auto U) { return f(KernelTag<gemm_fp8_splitk_kernel<MF, 1, 8, U>>{}, std::true_type{}), true; });
        return with_value<1, 2>(p.nf, [&](auto NF) {
            return with_value<4, 8>(p.nw, [&](auto NW) {
                return with_value<8, 16>(p.u, [&](auto U) { return f(KernelTag<gemm_bf16_splitk_kernel<MF, NF, NW, U>>{}, std::false_type{}), true; });
            });
        });
    });
}

// every split-K entry point: validate, plan, opt in, launch
int gemm_splitk(const SplitKCall& c) {
    if (const int rc = validate(c)) return rc;
    SplitKPlan p;
    if (const int rc = splitk_plan(c, p)) return rc;
    const int KS = c.K / c.ks;
    int rc = EAVQA_E_ARG;                                     // (no such variant: the plan and the dispatcher disagree)
    with_splitk_kernel(c.a_row_scale != nullptr, p, [&](auto k, auto fp8) {
        constexpr auto kernel = decltype(k)::value;
        if ((rc = opt_in_lds<kernel>(DECODE_LDS_MAX))) return;
        if constexpr (decltype(fp8)::value)
            hipLaunchKernelGGL(kernel, p.grid, dim3(p.block), p.lds, c.stream, reinterpret_cast<const unsigned char*>(c.A), c.lda, c.a_row_scale,
                               reinterpret_cast<const unsigned char*>(c.B), c.ldb, c.b_scale, c.partials, c.M, c.N, KS);
        else
            hipLaunchKernelGGL(kernel, p.grid, dim3(p.block), p.lds, c.stream, reinterpret_cast<const bf16_t*>(c.A), c.lda,
                               reinterpret_cast<const bf16_t*>(c.B), c.ldb, c.partials, c.M, c.N, KS);
        rc = hipGetLastError() != hipSuccess ? EAVQA_E_LAUNCH : EAVQA_OK;
    });
    return rc;
}

}  // namespace

extern "C" int eavqa_gemm_splitk_plan(int M, int N, int K) { return splitk_ks(false, M, N, K); }
extern "C" int eavqa_gemm_fp8_splitk_plan(int M, int N, int K) { return splitk_ks(true, M, N, K); }

extern "C" int eavqa_gemm_splitk_ex(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb,
                                    float* partials, int ks, void* stream, int unroll) {
    SplitKCall c;
    c.dtype = dtype; c.M = M; c.N = N; c.K = K; c.A = A; c.lda = lda; c.B = B; c.ldb = ldb; c.partials = partials; c.ks = ks;
    c.stream = reinterpret_cast<hipStream_t>(stream); c.sel = unroll;
    return gemm_splitk(c);
}

extern "C" int eavqa_gemm_splitk(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb,
                                 float* partials, int ks, void* stream) {
    return eavqa_gemm_splitk_ex(dtype, M, N, K, A, lda, B, ldb, partials, ks, stream, 0);
}

extern "C" int eavqa_gemm_fp8_splitk(int M, int N, int K, const void* A, int64_t lda, const float* a_row_scale, const void* B, int64_t ldb,
                                     float b_scale, float* partials, int ks, void* stream) {
    if (!a_row_scale) return EAVQA_E_ARG;
    SplitKCall c;
    c.M = M; c.N = N; c.K = K; c.A = A; c.lda = lda; c.a_row_scale = a_row_scale; c.B = B; c.ldb = ldb; c.b_scale = b_scale;
    c.partials = partials; c.ks = ks; c.stream = reinterpret_cast<hipStream_t>(stream);
    return gemm_splitk(c);
}

// The plan of a shape, for the tests (include/eavqa_test.h): validate() on a call of that shape whose pointers and leading dimensions
// are in order, then splitk_plan().  variant = (MF, NF, NW, U).
extern "C" int eavqa_gemm_splitk_route(int fp8, int M, int N, int K, int ks, int sel, eavqa_launch_plan_t* out) {
    float* const some = reinterpret_cast<float*>(uintptr_t(16));      // (aligned, never dereferenced)
    SplitKCall c;
    c.M = M; c.N = N; c.K = K; c.ks = ks; c.sel = sel; c.lda = c.ldb = K;
    c.A = c.B = c.partials = some;
    if (fp8) c.a_row_scale = some;
    if (const int rc = validate(c)) return rc;
    SplitKPlan p;
    if (const int rc = splitk_plan(c, p)) return rc;
    report(out, p.mf, p.nf, p.nw, p.u, p.grid, p.block, p.lds);
    return EAVQA_OK;
}

extern "C" int eavqa_splitk_finish(int dtype, int M, int N, const float* partials, int ks, const float* bias, int act,
                                   const float* residual, int64_t ld_residual, int out_f32, int n_seg,
                                   void* out0, int64_t ld0, void* out1, int64_t ld1, void* out2, int64_t ld2, void* stream) {
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (!partials || !out0 || M <= 0 || N <= 0 || ks <= 0 || n_seg < 1 || n_seg > 3) return EAVQA_E_ARG;
    if ((n_seg > 1 && !out1) || (n_seg > 2 && !out2)) return EAVQA_E_ARG;
    if (N % (4 * n_seg) || ld0 % 4 || (n_seg > 1 && ld1 % 4) || (n_seg > 2 && ld2 % 4) || (residual && ld_residual % 4)) return EAVQA_E_SHAPE;
    if (act < EAVQA_ACT_NONE || act > EAVQA_ACT_QUICK_GELU) return EAVQA_E_DTYPE;
    const int seg_cols = N / n_seg;
    const FinishSeg s0{out0, ld0}, s1{out1, ld1}, s2{out2, ld2};
    const int threads = M * (N / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_BF16)
        hipLaunchKernelGGL(splitk_finish_kernel<bf16_t>, dim3((threads + 255) / 256), dim3(256), 0, s, M, N, partials, ks, bias, act,
                           residual, ld_residual, out_f32, seg_cols, s0, s1, s2);
    else
        hipLaunchKernelGGL(splitk_finish_kernel<float>, dim3((threads + 255) / 256), dim3(256), 0, s, M, N, partials, ks, bias, act,
                           residual, ld_residual, 1, seg_cols, s0, s1, s2);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_splitk_finish_gated(int dtype, int M, int F, const float* partials, int ks, int act, void* out, int64_t ld, void* stream) {
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (!partials || !out || M <= 0 || F <= 0 || ks <= 0) return EAVQA_E_ARG;
    if (F % 4 || ld % 4) return EAVQA_E_SHAPE;
    if (act < EAVQA_ACT_NONE || act > EAVQA_ACT_QUICK_GELU) return EAVQA_E_DTYPE;
    const int threads = M * (F / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_BF16)
        hipLaunchKernelGGL(splitk_finish_gated_kernel<bf16_t>, dim3((threads + 255) / 256), dim3(256), 0, s, M, F, partials, ks, act,
                           reinterpret_cast<bf16_t*>(out), ld);
    else
        hipLaunchKernelGGL(splitk_finish_gated_kernel<float>, dim3((threads + 255) / 256), dim3(256), 0, s, M, F, partials, ks, act,
                           reinterpret_cast<float*>(out), ld);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
