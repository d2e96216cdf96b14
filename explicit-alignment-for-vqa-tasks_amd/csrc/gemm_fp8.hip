// fp8 (OCP e4m3) GEMM on the block-scaled matrix instruction (included by gemm.hip behind gemm_k64.hip).
//
// BASELINE.json configs[4] ("CLIP ViT-L/14 -> OPT-6.7B fp8 MFMA"): the frozen LM's Linear layers run on
// v_mfma_scale_f32_16x16x128_f8f6f4 - per MI355X_MICROARCH.md ("Matrix cores") only the block-scaled forms run at twice the bf16
// rate; the plain _fp8_fp8 MFMAs run at the bf16 rate.  Quantisation scheme (what the parity test's oracle reproduces):
//   * weights: e4m3 with ONE float scale per tensor, quantised once at load (frozen);
//   * activations / gradients: e4m3 with one float scale per ROW (token), produced by eavqa_quantize_rows_fp8 right before the
//     GEMM (dynamic, amax / 448; the contract of a quantised row is stated above the two kernels at the end of this file);
//   * the instruction's own E8M0 block scales are all 1.0 (exponent byte 127): the row and tensor scales are applied to the
//     fp32 accumulator in the epilogue (row_scale[m] * alpha), then bias / activation / residual as in eavqa_gemm.
// Structure: the loader / consumer specialised full-line kernel of gemm_k64.hip with byte-addressed operands - a stage row is
// 128 bytes = 128 fp8 k-values = ONE 16x16x128 MFMA step.  Lane (row r = lane & 15, group g = lane >> 4) of a fragment reads the
// 16-byte chunks g and g + 4 of its row (the two conflict-free reads of the bf16 kernel's two sub-steps) - i.e. the MFMA's
// k-group g holds k-values {16g .. 16g+15} and {64+16g .. 64+16g+15} of the stage, the same for A and for B, which permutes the
// terms of the dot product and nothing else.
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

template <int WM, int WN, int MF, int NF, int NST, int LW, bool DB>
__global__ __launch_bounds__(64 * (WM * WN + LW)) void gemm_fp8_k128s_kernel(GemmParamsBase pk, int gx, int gy, int tiles_m, int tiles_n) {
    const GemmParams p = widen(pk);
    using G = K64SGeo<WM, WN, MF, NF, NST, LW>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int tm, tn;
    if (!shaped_tile(gx, gy, tiles_m, tiles_n, tm, tn)) return;
    const int m0 = tm * G::TBM, n0 = tn * G::TBN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = p.K >> 7;                                                // 128 fp8 values per stage row
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wm = wave / WN, wn = wave % WN;

    if (wave >= G::NC) {
        k64s_loader_role<G>(reinterpret_cast<const char*>(p.A), reinterpret_cast<const char*>(p.B), p.lda, p.ldb, p.M, p.N, m0, n0, nk, smem,
                            wave - G::NC, lane);
    } else {
        const int frow = lane & 15, fk = lane >> 4;
        const int sw0 = ((fk ^ (frow & 7)) << 4);                           // chunk g; chunk g + 4 is sw0 ^ 64
        const int a_off = (wm * 16 * MF + frow) * 128;
        const int b_off = G::AOPER + (wn * 16 * NF + frow) * 128;
        constexpr int NSET = DB ? 2 : 1;
        i32x8 fa[NSET][MF], fb[NSET][NF];
        auto read_frags = [&](int set, const char* st) {
#pragma unroll
            for (int i = 0; i < MF; ++i) {
                const i32x4 lo = *reinterpret_cast<const i32x4*>(st + a_off + i * 2048 + sw0);
                const i32x4 hi = *reinterpret_cast<const i32x4*>(st + a_off + i * 2048 + (sw0 ^ 64));
                fa[set][i] = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const i32x4 lo = *reinterpret_cast<const i32x4*>(st + b_off + j * 2048 + sw0);
                const i32x4 hi = *reinterpret_cast<const i32x4*>(st + b_off + j * 2048 + (sw0 ^ 64));
                fb[set][j] = (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
        };
        auto mfma_all = [&](int set) {
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)      // cbsz = blgp = 0: both operands e4m3; block scales 2^0 (E8M0 byte 127 in every lane)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[set][i], fb[set][j], acc[i][j], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        };
        __builtin_amdgcn_s_barrier();                                       // tile 0 landed
        int stage = 0;
        if (DB) {
            read_frags(0, smem);
            for (int t = 0; t < nk; ++t) {
                const int nstage = (stage + 1 == NST) ? 0 : stage + 1;
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC07F);                         // lgkmcnt(0): fragments of tile t complete = done reading stage t
                if (t + 1 < nk) {
                    __builtin_amdgcn_s_barrier();                           // tile t+1 landed; the loader may refill stage t
                    if (t & 1) read_frags(0, smem + nstage * G::STAGE); else read_frags(1, smem + nstage * G::STAGE);
                }
                if (t & 1) mfma_all(1); else mfma_all(0);
                stage = nstage;
            }
        } else {
            for (int t = 0; t < nk; ++t) {
                __builtin_amdgcn_sched_barrier(0);
                read_frags(0, smem + stage * G::STAGE);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                if (t + 1 < nk) __builtin_amdgcn_s_barrier();
                mfma_all(0);
                stage = (stage + 1 == NST) ? 0 : stage + 1;
            }
        }
    }
    __syncthreads();
    k64s_store_tile<G, WM, WN, MF, NF>(p, acc, smem, wave, lane, m0, n0);
}

template <int WM, int WN, int MF, int NF, int NST, int LW, bool DB>
int launch_fp8(const GemmParams& p, hipStream_t stream) {
    using G = K64SGeo<WM, WN, MF, NF, NST, LW>;
    if (const int rc = opt_in_lds<gemm_fp8_k128s_kernel<WM, WN, MF, NF, NST, LW, DB>>(G::RING)) return rc;
    const int tiles_m = (p.M + G::TBM - 1) / G::TBM, tiles_n = (p.N + G::TBN - 1) / G::TBN;
    const GridPlan g = plan_grid(tiles_m, tiles_n, G::TBM, G::TBN);
    hipLaunchKernelGGL((gemm_fp8_k128s_kernel<WM, WN, MF, NF, NST, LW, DB>), dim3(g.per_xcd * 8), dim3(G::NT), G::RING, stream, p, g.gx, g.gy,
                       tiles_m, tiles_n);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

const K64Choice FP8_SHAPES[] = {
    {128, 80, 1, 1.56f, launch_fp8<4, 1, 2, 5, 4, 2, true>},
    {256, 128, 1, 1.97f, launch_fp8<4, 2, 4, 4, 3, 4, false>},
    {256, 160, 1, 1.93f, launch_fp8<4, 2, 4, 5, 3, 4, false>},
    {128, 128, 1, 1.73f, launch_fp8<2, 2, 4, 4, 3, 2, false>},
    {128, 256, 1, 1.97f, launch_fp8<2, 4, 4, 4, 3, 4, false>},
};
constexpr int N_FP8 = sizeof(FP8_SHAPES) / sizeof(FP8_SHAPES[0]);

// ---- row-wise quantisation: x[r, :] (bf16 or f32) -> e4m3 bytes + scale[r] = amax(|x[r, :]|) / 448 (1 where the row is all zero)
// The contract of a row, here and in the quantisers fused into the norm kernels (one rule: e4m3_row_scale / e4m3_pack4 of common.h;
// tests/_fp8_ref.py checks it against a float64 reference):
//   a row whose elements are all finite
//     * scale is a finite, positive, normal fp32: 1.0 exactly for an all-zero row, else max(fl32(amax * fl32(1/448)), 2^-126), so
//       |scale - amax / 448| <= 2^-23 scale whenever amax >= 448 * 2^-126;
//     * no byte is 0x7F / 0xFF; a zero element gives 0x00 / 0x80 (its sign); for amax >= 448 * 2^-126 an element of magnitude amax gives
//       0x7E / 0xFE;
//     * every byte is e4m3(x / (amax / 448)) rounded to nearest even from the float64 quotient, or the code next to it where that quotient
//       lies within a relative 2^-21 of the midpoint between the two (scale, reciprocal and product round half an fp32 ulp each);
//     * a row with 0 < amax < 448 * 2^-126 has scale 2^-126 and the bytes e4m3(x * 2^126), exactly (without the floor the reciprocal of
//       the scale overflowed below amax = 448 * 2^-128 and the whole row, zeros included, left as NaN bytes);
//   a row that holds a NaN or an infinity
//     * every non-finite element dequantises to a non-finite number (fmaxf drops a NaN from the amax; an infinite amax gives scale inf,
//       reciprocal 0 and inf * 0 = NaN); rows are independent, so every other row of the call is what it is without that row.
template <typename T>
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(int cols, const T* x, int64_t ldx, unsigned char* out, int64_t ld_out,
                                                                float* row_scale) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const T* xr = x + (int64_t)row * ldx;
    float amax = 0.f;
    for (int c = tid * 4; c < cols; c += 1024) {
        const float4 v = elem<T>::ld4(xr + c);
        amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float scale = e4m3_row_scale(amax);
    const float inv = 1.f / scale;
    if (tid == 0) row_scale[row] = scale;
    unsigned char* o = out + (int64_t)row * ld_out;
    for (int c = tid * 4; c < cols; c += 1024)         // second pass: the row is in L2
        *reinterpret_cast<int*>(o + c) = e4m3_pack4(elem<T>::ld4(xr + c), inv);
}

// bf16 rows of up to 2048 NV elements, 16-byte aligned: the row stays in registers between the amax pass and the conversion (one
// read of x, 16-byte loads, 8-byte stores); same arithmetic as the kernel above, so the bytes are identical.
template <int NV>
__global__ __launch_bounds__(256) void quantize_rows_fp8_reg_kernel(int cols, const bf16_t* __restrict__ x, int64_t ldx, unsigned char* __restrict__ out,
                                                                    int64_t ld_out, float* __restrict__ row_scale) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const bf16_t* xr = x + (int64_t)row * ldx;
    bf16x8 v[NV];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (tid + 256 * i) * 8;
        v[i] = (bf16x8){};
        if (c < cols) v[i] = *reinterpret_cast<const bf16x8*>(xr + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)v[i][e]));
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float scale = e4m3_row_scale(amax);
    const float inv = 1.f / scale;
    if (tid == 0) row_scale[row] = scale;
    unsigned char* o = out + (int64_t)row * ld_out;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (tid + 256 * i) * 8;
        if (c < cols) {
            const int lo = e4m3_pack4(make_float4((float)v[i][0], (float)v[i][1], (float)v[i][2], (float)v[i][3]), inv);
            const int hi = e4m3_pack4(make_float4((float)v[i][4], (float)v[i][5], (float)v[i][6], (float)v[i][7]), inv);
            *reinterpret_cast<int2*>(o + c) = make_int2(lo, hi);
        }
    }
}
