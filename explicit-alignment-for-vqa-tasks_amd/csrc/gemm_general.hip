// What every GEMM kernel shares - the block -> tile map, the eavqa_gemm_ln row statistics and the LDS-staged epilogue - and the general
// register-staged kernels, bf16 and f32, with their launcher (included by gemm.hip, inside its anonymous namespace; its head describes them).
constexpr int BM = 128, BN = 128;
constexpr int CS_PITCH = 132;                      // floats per row of the staged C tile
constexpr int CS_BYTES = BM * CS_PITCH * 4;         // 67,584 B

// XCD-aware, bijective block -> tile map: the dispatcher deals blocks round-robin over the
// 8 XCDs, so give each XCD a contiguous run of tiles (M fastest) to share operand panels in L2.
__device__ __forceinline__ void tile_coords(const GemmParams& p, int& tm, int& tn) {
    const int nwg = p.tiles_m * p.tiles_n;
    const int bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    tm = wgid % p.tiles_m;
    tn = wgid / p.tiles_m;
}

// eavqa_gemm_ln, consumer side: (rstd, -rstd mean) of the tile's rows from the producer's partial sums, once per tile.  Any subset of the
// workgroup's threads may run it (tid in [0, nthreads)); a barrier lies between it and the epilogue in every kernel.
__device__ __forceinline__ void ln_rowstat_fill(const GemmParams& p, float2* rowstat, int m0, int n0, int rows, int tid, int nthreads) {
    if (!p.ln_stats) return;
    for (int r = tid; r < rows; r += nthreads) {
        const int m = min(m0 + r, p.M - 1);
        const float2* q = reinterpret_cast<const float2*>(p.ln_stats) + (int64_t)m * p.ln_ld;
        float s = 0.f, ss = 0.f;
        if (((p.ln_ld | p.ln_parts) & 1) == 0 && (reinterpret_cast<uintptr_t>(p.ln_stats) & 15) == 0) {
            // two slots per 16-byte load, four loads in flight (a row's slots are contiguous); slots past the end are re-read from the last
            // pair and multiplied by zero, so the order of the additions does not depend on the slot count's remainder
            const float4* q4 = reinterpret_cast<const float4*>(q);
            const int n4 = p.ln_parts >> 1;
            for (int i = 0; i < n4; i += 4) {
                float4 t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) t[k] = q4[min(i + k, n4 - 1)];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float w = (i + k < n4) ? 1.f : 0.f;
                    s += w * (t[k].x + t[k].z);
                    ss += w * (t[k].y + t[k].w);
                }
            }
        } else {
            for (int i = 0; i < p.ln_parts; ++i) { const float2 t = q[i]; s += t.x; ss += t.y; }
        }
        const float mean = s * p.ln_inv_n;
        const float rstd = 1.0f / sqrtf(fmaxf(ss * p.ln_inv_n - mean * mean, 0.f) + p.ln_eps);
        rowstat[r] = make_float2(rstd, -rstd * mean);
        if (n0 == 0 && m0 + r < p.M && p.mean_out) { p.mean_out[m] = mean; p.rstd_out[m] = rstd; }
    }
}

// ---- epilogue shared by all kernels: Cs holds the 128x128 fp32 tile (pitch CS_PITCH) ----
// MODE: 0 = no activation, 1 = forward activation, 2 = multiply by the activation derivative at aux_in.
// FULL: the tile lies entirely inside C and every operand allows vector access: no bounds checks, 8/16-byte
// accesses only (every tile of the hot shapes except the last row of tiles).
// Geometry G: TPR threads cover one row of the staged tile (4 columns each), RPP rows per pass, NPASS passes, PITCH floats
// per staged row.
// ROWS < RPP * NPASS (tile widths that do not divide the block): threads beyond TPR * RPP idle, the last pass is cut at ROWS.
template <int TPR_, int RPP_, int NPASS_, int PITCH_, int ROWS_ = RPP_ * NPASS_, int LN_UNROLL_ = 4> struct EpiGeo {
    static constexpr int TPR = TPR_, RPP = RPP_, NPASS = NPASS_, PITCH = PITCH_, ROWS = ROWS_;
    static constexpr int LN_UNROLL = LN_UNROLL_;      // passes in flight in the eavqa_gemm_ln form of the epilogue (1 where registers are short)
};
using EpiGeo128 = EpiGeo<32, 8, 16, CS_PITCH>;      // 128 x 128 tile, 256 threads

// one row m, four consecutive columns n .. n + 3: v[] = the fp32 accumulators on entry
template <typename T, int ACT, int MODE, bool FULL, bool LNX>
__device__ __forceinline__ void epilogue_quad(const GemmParams& p, int m, int n, float (&v)[4], const float (&bias4)[4], const float2 rs,
                                              const float (&c4)[4]) {
    const T* aux_in = reinterpret_cast<const T*>(p.aux_in);
    T* aux_out = reinterpret_cast<T*>(p.aux_out);
    const bool full = FULL || (n + 3 < p.N);
    const float al = p.row_scale ? p.alpha * p.row_scale[m] : p.alpha;
    if (LNX && p.ln_stats) {                             // rstd (alpha acc - mean c[n]) + bias[n]
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (al * rs.x) * v[j] + (bias4[j] + rs.y * c4[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = al * v[j] + bias4[j];
    }
    if (aux_out) {
        T* q = aux_out + (int64_t)m * p.ld_aux + n;
        if (FULL || (full && p.vec_aux)) elem<T>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<T>::st(q + j, v[j]);
    }
    if (MODE == 2) {
        const T* q = aux_in + (int64_t)m * p.ld_aux + n;
        float u[4] = {0.f, 0.f, 0.f, 0.f};
        if (FULL || (full && p.vec_aux)) { float4 t = elem<T>::ld4(q); u[0] = t.x; u[1] = t.y; u[2] = t.z; u[3] = t.w; }
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) u[j] = elem<T>::ld(q + j);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= act_bwd(ACT, u[j]);
    } else if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_fwd(ACT, v[j]);
    }
    if (p.residual) {
        if (p.res_lowp == 2) {                             // 16-bit residual stream of a frozen tower (the CLIP tower): half ...
            const f16_t* q = reinterpret_cast<const f16_t*>(p.residual) + (int64_t)m * p.ldr + n;
            if (FULL || (full && p.vec_res)) { float4 t = elem<f16_t>::ld4(q); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            else
                for (int j = 0; j < 4; ++j)
                    if (n + j < p.N) v[j] += elem<f16_t>::ld(q + j);
        } else if (p.res_lowp) {                           // ... or the operand dtype
            const T* q = reinterpret_cast<const T*>(p.residual) + (int64_t)m * p.ldr + n;
            if (FULL || (full && p.vec_res)) { float4 t = elem<T>::ld4(q); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            else
                for (int j = 0; j < 4; ++j)
                    if (n + j < p.N) v[j] += elem<T>::ld(q + j);
        } else {
            const float* q = reinterpret_cast<const float*>(p.residual) + (int64_t)m * p.ldr + n;
            if (FULL || (full && p.vec_res)) { float4 t = *reinterpret_cast<const float4*>(q); v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
            else
                for (int j = 0; j < 4; ++j)
                    if (n + j < p.N) v[j] += q[j];
        }
    }
    if (p.out_f32) {
        float* q = reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n;
        if (FULL || (full && p.vec_c)) *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) q[j] = v[j];
    } else if (p.out_f16) {
        f16_t* q = reinterpret_cast<f16_t*>(p.C) + (int64_t)m * p.ldc + n;
        if (FULL || (full && p.vec_c)) elem<f16_t>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<f16_t>::st(q + j, v[j]);
    } else {
        T* q = reinterpret_cast<T*>(p.C) + (int64_t)m * p.ldc + n;
        if (FULL || (full && p.vec_c)) elem<T>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<T>::st(q + j, v[j]);
    }
    if (LNX && p.copy_out) {
        T* q = reinterpret_cast<T*>(p.copy_out) + (int64_t)m * p.ld_copy + n;
        if (full && p.vec_copy) elem<T>::st4(q, make_float4(v[0], v[1], v[2], v[3]));
        else
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) elem<T>::st(q + j, v[j]);
    }
}

template <bool FULL>
__device__ __forceinline__ void load_bias4(const GemmParams& p, int n, float (&bias4)[4]) {
    bias4[0] = bias4[1] = bias4[2] = bias4[3] = 0.f;
    if (p.bias) {
        if (FULL) { const float4 b = *reinterpret_cast<const float4*>(p.bias + n); bias4[0] = b.x; bias4[1] = b.y; bias4[2] = b.z; bias4[3] = b.w; }
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < p.N) bias4[j] = p.bias[n + j];
        }
    }
}

// LnArgs: where the tile's row statistics lie (eavqa_gemm_ln consumer side) and which of them this staged slab starts at
struct LnArgs { const float2* rowstat; int row_base; };

template <typename T, int ACT, int MODE, bool FULL, typename G, bool LNX>
__device__ __forceinline__ void epilogue_body(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln) {
    const int tid = threadIdx.x;
    if (G::ROWS != G::RPP * G::NPASS && tid >= G::TPR * G::RPP) return;
    const int c4 = (tid % G::TPR) * 4;
    const int n = n0 + c4;
    float bias4[4], lc4[4] = {0.f, 0.f, 0.f, 0.f};
    load_bias4<FULL>(p, n, bias4);
    if (LNX && p.ln_stats) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (FULL || n + j < p.N) lc4[j] = p.ln_c[n + j];
    }
    auto one_pass = [&](int pass) {
        const int row = (tid / G::TPR) + pass * G::RPP;
        const int m = m0 + row;
        if (G::ROWS != G::RPP * G::NPASS && row >= G::ROWS) return;
        if (!FULL && (m >= p.M || n >= p.N)) return;
        const float4 a = *reinterpret_cast<const float4*>(&Cs[row * G::PITCH + c4]);
        float v[4] = {a.x, a.y, a.z, a.w};
        const float2 rs = (LNX && p.ln_stats) ? ln.rowstat[ln.row_base + row] : make_float2(1.f, 0.f);
        epilogue_quad<T, ACT, MODE, FULL, LNX>(p, m, n, v, bias4, rs, lc4);
        if (LNX && p.stats_out) {                           // the values as stored (before any rounding), zeros beyond column N, back into the staged tile
            if (!FULL) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n + j >= p.N) v[j] = 0.f;
            }
            *reinterpret_cast<float4*>(&Cs[row * G::PITCH + c4]) = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    if constexpr (LNX && G::LN_UNROLL == 1) {               // (a literal count: the pragma does not take a dependent expression reliably)
#pragma unroll 1
        for (int pass = 0; pass < G::NPASS; ++pass) one_pass(pass);
    } else {
#pragma unroll 4
        for (int pass = 0; pass < G::NPASS; ++pass) one_pass(pass);
    }
}

// eavqa_gemm_ln, producer side: (sum, sum of squares) of the finished rows of this slab, one thread per row in column order (a fixed
// summation order: bitwise reproducible), into the 64-column slots the tile covers - the whole sum in the first, zeros in the others -
// and zeros into the slots behind the last tile column, so that a consumer adds all stats_ld slots without knowing the tile width.
template <typename G>
__device__ __forceinline__ void epilogue_row_sums(const GemmParams& p, const float* Cs, int m0, int n0) {
    constexpr int COLS = G::TPR * 4;
    static_assert(COLS >= 64 && COLS % 4 == 0, "a tile covers at least one 64-column slot");
    __syncthreads();
    const int cols = min(COLS, p.N - n0);
    const int slot0 = n0 / 64, slot1 = (n0 + COLS < p.N) ? (n0 + COLS) / 64 : p.stats_ld;     // this tile owns slots [slot0, slot1)
    for (int r = threadIdx.x; r < G::ROWS; r += blockDim.x) {
        const int m = m0 + r;
        if (m >= p.M) continue;
        float s = 0.f, ss = 0.f;
        for (int c = 0; c < cols; c += 4) {
            const float4 t = *reinterpret_cast<const float4*>(&Cs[r * G::PITCH + c]);
            s += (t.x + t.y) + (t.z + t.w);
            ss += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
        }
        float2* q = reinterpret_cast<float2*>(p.stats_out) + (int64_t)m * p.stats_ld;
        q[slot0] = make_float2(s, ss);
        for (int i = slot0 + 1; i < slot1; ++i) q[i] = make_float2(0.f, 0.f);
    }
}

template <typename T, int ACT, int MODE, typename G, bool LNX>
__device__ __forceinline__ void epilogue_mode(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln) {
    constexpr int ROWS = G::ROWS, COLS = G::TPR * 4;
    const bool full_tile = (m0 + ROWS <= p.M) && (n0 + COLS <= p.N) && p.vec_c && (!(p.aux_in || p.aux_out) || p.vec_aux) &&
                           (!p.residual || p.vec_res) && (!p.bias || p.vec_bias);
    if (full_tile) epilogue_body<T, ACT, MODE, true, G, LNX>(p, Cs, m0, n0, ln);
    else epilogue_body<T, ACT, MODE, false, G, LNX>(p, Cs, m0, n0, ln);
    if (LNX && p.stats_out) epilogue_row_sums<G>(p, Cs, m0, n0);
}

// block-uniform dispatch on the (runtime) activation id / mode: each combination gets its own straight-line body
// LNX = false compiles the eavqa_gemm_ln paths out (the 1024-thread 256 x 256 kernel has 128 registers per lane: its plain form must not carry them)
template <typename T, typename G = EpiGeo128, bool LNX = true>
__device__ __forceinline__ void epilogue(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln = LnArgs{nullptr, 0}) {
    const int mode = p.aux_in ? 2 : (p.act != EAVQA_ACT_NONE ? 1 : 0);
    if (mode == 0) { epilogue_mode<T, EAVQA_ACT_NONE, 0, G, LNX>(p, Cs, m0, n0, ln); return; }
    switch (p.act) {
        case EAVQA_ACT_TANH:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_TANH, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_TANH, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        case EAVQA_ACT_RELU:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_RELU, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_RELU, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        case EAVQA_ACT_GELU_NEW:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_GELU_NEW, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_GELU_NEW, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        case EAVQA_ACT_QUICK_GELU:
            if (mode == 1) epilogue_mode<T, EAVQA_ACT_QUICK_GELU, 1, G, LNX>(p, Cs, m0, n0, ln); else epilogue_mode<T, EAVQA_ACT_QUICK_GELU, 2, G, LNX>(p, Cs, m0, n0, ln);
            break;
        default:   // aux_in with act == none: derivative 1
            epilogue_mode<T, EAVQA_ACT_NONE, 0, G, LNX>(p, Cs, m0, n0, ln);
    }
}

// the call every kernel with registers to spare makes: the plain epilogue unless the launch carries eavqa_gemm_ln arguments (block-uniform)
template <typename T, typename G = EpiGeo128>
__device__ __forceinline__ void epilogue_any(const GemmParams& p, float* Cs, int m0, int n0, const LnArgs ln = LnArgs{nullptr, 0}) {
    if (p.ln_stats || p.stats_out || p.copy_out) epilogue<T, G, true>(p, Cs, m0, n0, ln);
    else epilogue<T, G, false>(p, Cs, m0, n0, ln);
}

// (Round 3 built a direct register -> global epilogue for the specialised tiles - operands swapped, B fragment rows permuted so that a
// lane owns 16 consecutive columns - and measured it 10-70 % SLOWER than the LDS-staged pass below (a wave's store covers 16 rows x
// 32 bytes: partial lines); removed again, numbers in profiles/round3_direct_epilogue.md.)

// =============================================================== bf16 ===
constexpr int BK16 = 64;                          // k per LDS tile (bf16)
constexpr int OPER16_BYTES = 128 * BK16 * 2;      // 16 KiB per operand per buffer

// byte offset of the 16-byte chunk (row, kc) inside a swizzled [128][64] bf16 tile
__device__ __forceinline__ int swz16(int row, int kc) { return row * 128 + ((kc ^ (row & 7)) << 4); }

// Stage one operand tile (128 rows x 64 k) from global memory into registers.
// KC: memory is [rows][K] (k contiguous); else memory is [K][rows] (row contiguous).
template <bool KC>
__device__ __forceinline__ void g2r_16(uint4 (&r)[4], const bf16_t* X, int64_t ld, int row0, int rows_max,
                                       int k0, int K) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (KC) {
            const int row = c >> 3, kc = c & 7;
            const int gr = row0 + row, gk = k0 + kc * 8;
            if (gr < rows_max && gk < K) v = *reinterpret_cast<const uint4*>(X + (int64_t)gr * ld + gk);
        } else {
            const int k = c >> 4, rc = c & 15;
            const int gk = k0 + k, gr = row0 + rc * 8;
            if (gk < K && gr < rows_max) v = *reinterpret_cast<const uint4*>(X + (int64_t)gk * ld + gr);
        }
        r[i] = v;
    }
}
template <bool KC>
__device__ __forceinline__ void r2s_16(const uint4 (&r)[4], char* S) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i;
        if (KC) {
            const int row = c >> 3, kc = c & 7;
            *reinterpret_cast<uint4*>(S + swz16(row, kc)) = r[i];
        } else {
            const int k = c >> 4, rc = c & 15;
            const unsigned w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = rc * 8 + j;
                const unsigned short e = (unsigned short)((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu));
                *reinterpret_cast<unsigned short*>(S + swz16(row, k >> 3) + (k & 7) * 2) = e;
            }
        }
    }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS carve: A buffers at 0 / 16 KiB, B buffers at 32 / 48 KiB (pointer arrays of LDS addresses
    // would become static initialisers, which the backend rejects - use offsets)
    char* const As0 = smem;
    char* const Bs0 = smem + 2 * OPER16_BYTES;

    int tm, tn;
    tile_coords(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = (p.K + BK16 - 1) / BK16;
    uint4 ra[4], rb[4];
    g2r_16<A_KC>(ra, A, p.lda, m0, p.M, 0, p.K);
    g2r_16<B_KC>(rb, B, p.ldb, n0, p.N, 0, p.K);
    r2s_16<A_KC>(ra, As0);
    r2s_16<B_KC>(rb, Bs0);
    __syncthreads();

    const int frow = lane & 15, fk = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            g2r_16<A_KC>(ra, A, p.lda, m0, p.M, (kt + 1) * BK16, p.K);
            g2r_16<B_KC>(rb, B, p.ldb, n0, p.N, (kt + 1) * BK16, p.K);
        }
        const char* Ac = As0 + cur * OPER16_BYTES;
        const char* Bc = Bs0 + cur * OPER16_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm * 64 + i * 16 + frow;
                af[i] = *reinterpret_cast<const bf16x8*>(Ac + swz16(row, s * 4 + fk));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wn * 64 + j * 16 + frow;
                bfr[j] = *reinterpret_cast<const bf16x8*>(Bc + swz16(row, s * 4 + fk));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) {
            r2s_16<A_KC>(ra, As0 + (cur ^ 1) * OPER16_BYTES);
            r2s_16<B_KC>(rb, Bs0 + (cur ^ 1) * OPER16_BYTES);
        }
        __syncthreads();
    }

    // accumulators -> LDS (C/D map of 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg)
    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                const int col = wn * 64 + j * 16 + (lane & 15);
                Cs[row * CS_PITCH + col] = acc[i][j][r];
            }
    float2* rowstat = reinterpret_cast<float2*>(smem + CS_BYTES);          // present when launched with ln_lds(p) extra bytes
    ln_rowstat_fill(p, rowstat, m0, n0, BM, tid, 256);
    __syncthreads();
    if constexpr (A_KC && B_KC) epilogue_any<bf16_t>(p, Cs, m0, n0, LnArgs{rowstat, 0});       // (the other layouts do without the eavqa_gemm_ln form: compile time)
    else epilogue<bf16_t, EpiGeo128, false>(p, Cs, m0, n0);
}

// ================================================================ f32 ===
constexpr int BK32 = 16;
constexpr int PITCH32 = 17;                                  // floats per staged row
constexpr int OPER32_FLOATS = 128 * PITCH32;                 // 2176 floats = 8704 B

template <bool KC>
__device__ __forceinline__ void g2r_32(float4 (&r)[2], const float* X, int64_t ld, int row0, int rows_max,
                                       int k0, int K) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (KC) {
            const int row = c >> 2, kc = c & 3;
            const int gr = row0 + row, gk = k0 + kc * 4;
            if (gr < rows_max && gk < K) v = *reinterpret_cast<const float4*>(X + (int64_t)gr * ld + gk);
        } else {
            const int k = c >> 5, rc = c & 31;
            const int gk = k0 + k, gr = row0 + rc * 4;
            if (gk < K && gr < rows_max) v = *reinterpret_cast<const float4*>(X + (int64_t)gk * ld + gr);
        }
        r[i] = v;
    }
}
template <bool KC>
__device__ __forceinline__ void r2s_32(const float4 (&r)[2], float* S) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i;
        const float w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
        if (KC) {
            const int row = c >> 2, kc = c & 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) S[row * PITCH32 + kc * 4 + j] = w[j];
        } else {
            const int k = c >> 5, rc = c & 31;
#pragma unroll
            for (int j = 0; j < 4; ++j) S[(rc * 4 + j) * PITCH32 + k] = w[j];
        }
    }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sm = reinterpret_cast<float*>(smem);
    float* const As0 = sm;
    float* const Bs0 = sm + 2 * OPER32_FLOATS;

    int tm, tn;
    tile_coords(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const float* A = reinterpret_cast<const float*>(p.A);
    const float* B = reinterpret_cast<const float*>(p.B);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (p.K + BK32 - 1) / BK32;
    float4 ra[2], rb[2];
    g2r_32<A_KC>(ra, A, p.lda, m0, p.M, 0, p.K);
    g2r_32<B_KC>(rb, B, p.ldb, n0, p.N, 0, p.K);
    r2s_32<A_KC>(ra, As0);
    r2s_32<B_KC>(rb, Bs0);
    __syncthreads();

    const int frow = lane & 31, fk = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            g2r_32<A_KC>(ra, A, p.lda, m0, p.M, (kt + 1) * BK32, p.K);
            g2r_32<B_KC>(rb, B, p.ldb, n0, p.N, (kt + 1) * BK32, p.K);
        }
        const float* Ac = As0 + cur * OPER32_FLOATS;
        const float* Bc = Bs0 + cur * OPER32_FLOATS;
#pragma unroll
        for (int s = 0; s < BK32 / 2; ++s) {
            float af[2], bfr[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = Ac[(wm * 64 + i * 32 + frow) * PITCH32 + s * 2 + fk];
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = Bc[(wn * 64 + j * 32 + frow) * PITCH32 + s * 2 + fk];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) {
            r2s_32<A_KC>(ra, As0 + (cur ^ 1) * OPER32_FLOATS);
            r2s_32<B_KC>(rb, Bs0 + (cur ^ 1) * OPER32_FLOATS);
        }
        __syncthreads();
    }

    // C/D map of 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int col = wn * 64 + j * 32 + (lane & 31);
                Cs[row * CS_PITCH + col] = acc[i][j][r];
            }
    float2* rowstat = reinterpret_cast<float2*>(smem + CS_BYTES);          // present when launched with ln_lds(p) extra bytes
    ln_rowstat_fill(p, rowstat, m0, n0, BM, tid, 256);
    __syncthreads();
    if constexpr (A_KC && B_KC) epilogue_any<float>(p, Cs, m0, n0, LnArgs{rowstat, 0});
    else epilogue<float, EpiGeo128, false>(p, Cs, m0, n0);
}

template <auto Kernel> int launch_general(const GemmParams& p, hipStream_t stream) {
    if (const int rc = opt_in_lds<Kernel>(CS_BYTES + LN_ROWSTAT_BYTES)) return rc;
    const int nwg = p.tiles_m * p.tiles_n;
    hipLaunchKernelGGL(Kernel, dim3(nwg), dim3(256), CS_BYTES + ln_lds(p), stream, p);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
