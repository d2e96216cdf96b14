// The round-1 LDS-DMA family of bf16 kernels (BK = 32 ring, included by gemm.hip inside its anonymous namespace): the 128 x 128 fast kernel,
// the shaped tiles, the 256 x 256 kernel, their grid planners and the cost models the dispatcher ranks them with.
// ===================================================== bf16 fast path ===
// Both operands k-contiguous and K % 32 == 0 (every GEMM of the frozen ViT / LM, forward and dgrad,
// after weight pre-packing).  Differences from the general kernel above:
//   * global -> LDS by LDS-DMA (global_load_lds_dwordx4): no staging registers, no ds_write;
//   * BK = 32, a ring of 4 LDS stages (16 KiB each: A 8 KiB + B 8 KiB), tiles t+1..t+3 in flight
//     while tile t is multiplied; ONE raw s_barrier per K-tile with a counted vmcnt (never 0 in
//     the steady state), so the DMA stays in flight across barriers;
//   * 64-byte LDS rows with the 16-byte chunk XOR-swizzled by (-(row >> 2)) & 3: the 16 lanes of
//     every ds_read_b128 lane group land on 16 different 16-byte slots of the 256-byte bank row.
//     LDS-DMA writes linearly (wave base + lane * 16), so the swizzle is applied to the per-lane
//     SOURCE address and again on the fragment read (same involution);
//   * rows beyond M / N are clamped to the last valid row (their products only reach output rows
//     that are never stored), so no lane is predicated off and the DMA count per wave is exact;
//   * the LDS footprint (ring 64 KiB, C staging 66 KiB) lets two workgroups share a CU;
//   * block -> tile map: each XCD (blockIdx % 8) owns a rectangle of the tile grid so that the
//     A / B panels it re-reads stay in its own 4 MiB L2.
constexpr int FBK = 32;
constexpr int FOPER = 128 * FBK * 2;        // 8 KiB per operand per stage
constexpr int FSTAGE = 2 * FOPER;           // 16 KiB

__device__ __forceinline__ int fswz(int row, int kc) { return row * 64 + ((kc ^ ((-(row >> 2)) & 3)) << 4); }

struct FastMap { int gx, gy; };

__device__ __forceinline__ bool fast_tile(const GemmParams& p, int gx, int gy, int& tm, int& tn) {
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int xi = xcd % gx, yi = xcd / gx;
    const int qm = p.tiles_m / gx, rm = p.tiles_m % gx, qn = p.tiles_n / gy, rn = p.tiles_n % gy;
    const int m_begin = xi * qm + min(xi, rm), m_cnt = qm + (xi < rm ? 1 : 0);
    const int n_begin = yi * qn + min(yi, rn), n_cnt = qn + (yi < rn ? 1 : 0);
    if (m_cnt == 0 || local >= m_cnt * n_cnt) return false;
    tm = m_begin + local % m_cnt;
    tn = n_begin + local / m_cnt;
    return true;
}

// one pipeline step: tile t is already in registers (fragment set P); tile t+1 is fetched from its LDS stage
// into set P^1 while the 16 MFMAs of tile t run, and the DMA of tile t+4 is issued into the stage tile t
// occupied (its fragments left LDS during the previous step).
#define EAVQA_FAST_STEP(P, t)                                                                         \
    {                                                                                                 \
        const int rem = nk - 2 - (t);             /* tiles issued after t+1 */                         \
        /* fragment set P (read during the previous step) is complete; unconditional so that the      */ \
        /* compiler's own lgkmcnt bookkeeping sees it on every path and adds no drain before the MFMAs */ \
        /* sched_barrier: MFMAs are register-only, so the scheduler would otherwise sink the previous  */ \
        /* step's MFMAs below this wait (draining the reads that were just issued)                    */ \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        __builtin_amdgcn_s_waitcnt(0xC07F);       /* lgkmcnt(0) */                                     \
        if ((t) + 1 < nk) {                                                                           \
            /* s_waitcnt simm16 (gfx9): vmcnt [3:0]+[15:14], expcnt [6:4], lgkmcnt [11:8]; the builtin   */ \
            /* (unlike inline asm) is seen by the compiler's own wait-count bookkeeping.  Tiles t+2 ..   */ \
            /* t+NST-1 (4 DMA each) may stay in flight; near the end fewer were issued.                 */ \
            if (ABL < 3) {                                                                            \
            if (rem >= NST - 2) __builtin_amdgcn_s_waitcnt(vm_only(4 * (NST - 2)));                   \
            else if (rem >= 6) __builtin_amdgcn_s_waitcnt(vm_only(24));                               \
            else if (rem == 5) __builtin_amdgcn_s_waitcnt(vm_only(20));                               \
            else if (rem == 4) __builtin_amdgcn_s_waitcnt(vm_only(16));                               \
            else if (rem == 3) __builtin_amdgcn_s_waitcnt(vm_only(12));                               \
            else if (rem == 2) __builtin_amdgcn_s_waitcnt(vm_only(8));                                \
            else if (rem == 1) __builtin_amdgcn_s_waitcnt(vm_only(4));                                \
            else __builtin_amdgcn_s_waitcnt(vm_only(0));                                              \
            __builtin_amdgcn_s_barrier();                                                             \
            }                                                                                         \
            if ((ABL < 1 || ABL >= 4) && (t) + NST < nk) issue((t) + NST);                            \
            if (ABL < 2) {                                                                            \
            const char* st = smem + (((t) + 1) & (NST - 1)) * FSTAGE;                                 \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                             \
                fa[(P) ^ 1][i] = *reinterpret_cast<const bf16x8*>(st + a_off + i * 1024);             \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                             \
                fb[(P) ^ 1][j] = *reinterpret_cast<const bf16x8*>(st + b_off + j * 1024);             \
            } else {                                                                                  \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) { fa[(P) ^ 1][i] = fa[P][i]; fb[(P) ^ 1][i] = fb[P][i]; } \
            }                                                                                         \
        }                                                                                             \
        if (ABL != 4) {                                                                               \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                 \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                             \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[P][i], fb[P][j], acc[i][j], 0, 0, 0); \
        }                                                                                             \
    }

// s_waitcnt immediate for "vmcnt(n) only" (lgkmcnt and expcnt fields at their no-wait maxima)
__device__ __host__ constexpr int vm_only(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }

// NST: stages of the LDS ring (4: 64 KiB, two workgroups per CU; 8: 128 KiB, used when the grid has at most one
// workgroup per CU anyway - twice the bytes in flight per CU lifts the latency-bound LDS-DMA rate).
// ABL (timing experiments only, results are wrong for ABL != 0): 1 = no DMA in the main loop, 2 = also no
// fragment reads, 3 = also no barrier / waits (bare MFMA loop), 4 = DMA + waits + barriers only (no reads, no MFMA)
template <int ABL, int NST>
__global__ __launch_bounds__(256, 2) void gemm_bf16_fast_kernel(GemmParams p, int gx, int gy, int stagger) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int tm, tn;
    if (!fast_tile(p, gx, gy, tm, tn)) return;
    // two workgroups share a CU and would otherwise run in lockstep (same program, same start): delay every
    // other one so that one block's MFMA phase overlaps the other's DMA-issue / LDS-read phase
    if (stagger > 0 && ((blockIdx.x >> 3) & 1))
        for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(8);
    const int m0 = tm * BM, n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    // per-lane DMA sources: chunk c = wave*64 + lane + 256*i of the [128 rows][4 chunks] image
    const bf16_t* asrc[2];
    const bf16_t* bsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i;
        const int row = c >> 2, pc = c & 3;
        const int kc = pc ^ ((-(row >> 2)) & 3);
        asrc[i] = A + (int64_t)min(m0 + row, p.M - 1) * p.lda + kc * 8;
        bsrc[i] = B + (int64_t)min(n0 + row, p.N - 1) * p.ldb + kc * 8;
    }
    const int dma_off = wave * 1024;     // wave-uniform LDS offset of this wave's 64 chunks

    auto issue = [&](int kt) {
        char* st = smem + (kt & (NST - 1)) * FSTAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off + i * 4096), 16, 0, 0);
            if (ABL != 5 || i == 0 || lane < 16)     // ABL 5: the DMA pattern of a 128 x 80 tile (quarter-wave last piece)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + FOPER + dma_off + i * 4096), 16, 0, 0);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / FBK;
    const int frow = lane & 15, fk = lane >> 4;
    const int a_off = fswz(wm * 64 + frow, fk);          // + i * 16 rows * 64 B
    const int b_off = FOPER + fswz(wn * 64 + frow, fk);
    bf16x8 fa[2][4], fb[2][4];

    // prologue: tiles 0..NST-1 in flight, tile 0 into fragment set 0
#pragma unroll
    for (int i = 0; i < NST; ++i)
        if (i < nk) issue(i);
    {
        const int later = min(nk, NST) - 1;              // tiles issued after tile 0
        if (later >= 7) __builtin_amdgcn_s_waitcnt(vm_only(28));
        else if (later == 6) __builtin_amdgcn_s_waitcnt(vm_only(24));
        else if (later == 5) __builtin_amdgcn_s_waitcnt(vm_only(20));
        else if (later == 4) __builtin_amdgcn_s_waitcnt(vm_only(16));
        else if (later == 3) __builtin_amdgcn_s_waitcnt(vm_only(12));
        else if (later == 2) __builtin_amdgcn_s_waitcnt(vm_only(8));
        else if (later == 1) __builtin_amdgcn_s_waitcnt(vm_only(4));
        else __builtin_amdgcn_s_waitcnt(vm_only(0));
    }
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[0][i] = *reinterpret_cast<const bf16x8*>(smem + a_off + i * 1024);
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[0][j] = *reinterpret_cast<const bf16x8*>(smem + b_off + j * 1024);

    int t = 0;
    for (; t + 1 < nk; t += 2) {
        EAVQA_FAST_STEP(0, t)
        EAVQA_FAST_STEP(1, t + 1)
    }
    if (t < nk) EAVQA_FAST_STEP(0, t)
    __syncthreads();   // every wave is done with the ring before it becomes the C staging tile

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
    __syncthreads();
    epilogue<bf16_t, EpiGeo128, false>(p, Cs, m0, n0);
}
#undef EAVQA_FAST_STEP


typedef void (*fast_kernel_t)(GemmParams, int, int, int);

int launch_fast(const GemmParams& p, hipStream_t stream, const Knobs& kn) {
    // (round 3: the timing-only ablation builds ABL 1..5 of this round-1 kernel are no longer instantiated; the knob field is ignored here)
    // deep ring (8 stages, one workgroup per CU): measured on MI355X to give no gain over 4 stages even for grids of one
    // tile per CU (the LDS-DMA rate of a CU is a throughput cap, not a bytes-in-flight limit) - kept as an experiment knob
    const bool deep = kn.deep == 2;
    const fast_kernel_t kernel = deep ? gemm_bf16_fast_kernel<0, 8> : gemm_bf16_fast_kernel<0, 4>;
    if (const int rc = deep ? opt_in_lds<gemm_bf16_fast_kernel<0, 8>>(8 * FSTAGE) : opt_in_lds<gemm_bf16_fast_kernel<0, 4>>(8 * FSTAGE)) return rc;
    const int lds_bytes = deep ? 8 * FSTAGE : CS_BYTES;
    // XCD grid gx x gy = 8 minimising the panels one XCD touches (rows + cols of its rectangle)
    int best_gx = 8, best_cost = 1 << 30;
    const int cand[4] = {8, 4, 2, 1};
    for (int c = 0; c < 4; ++c) {
        const int gx = cand[c], gy = 8 / gx;
        const int cost = (p.tiles_m + gx - 1) / gx + (p.tiles_n + gy - 1) / gy;
        if (cost < best_cost) { best_cost = cost; best_gx = gx; }
    }
    const int gx = best_gx, gy = 8 / gx;
    const int per_xcd = ((p.tiles_m + gx - 1) / gx) * ((p.tiles_n + gy - 1) / gy);
    hipLaunchKernelGGL(kernel, dim3(per_xcd * 8), dim3(256), lds_bytes, stream, p, gx, gy, kn.stagger);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}


// ============================================== bf16 shaped tiles ===
// (16 MF WM) x (16 NF WN) output tile per workgroup of WM x WN waves, same LDS-DMA ring (BK = 32, 4 stages, counted vmcnt,
// one s_barrier per K-step) and register-prefetched fragments as the fast kernel.  Why other shapes: a CU takes in its
// operand tiles at a fixed rate (measured ~52 GB/s into LDS whether one or two workgroups share the CU: K = 5120 takes
// 50 / 51 / 54 us on 80 / 160 / 256 tiles of 128 x 128 and 103 us on 512), so the time of a GEMM is
//     rounds of 256 workgroups  x  (BM + BN) bytes per workgroup and K-step
// and the best tile is the one whose grid just fills the 256 CUs once:
//   * narrow 128 x 80 / 128 x 96 (4 x 1 waves, 2 x NF fragments): N = 1280 at M ~ 2000 is 160 tiles of 128 x 128 (96 CUs
//     idle) but 256 tiles of 128 x 80, each moving 208 / 256 of the bytes;
//   * tall 256 x 128 / 256 x 160 / 256 x 192 (4 x 2 waves, 4 x NF fragments): N = 3840 at M ~ 2000 is 480 tiles of
//     128 x 128 (two rounds) but 240 of 256 x 128 (one round at 384 / 512 of the bytes).
// The B stage (16 NF WN rows x 64 B) is moved by BFULL full-wave DMAs per wave plus, when 4 BN is not a multiple of the
// workgroup size, one piece of BREM lanes per wave, so that every wave issues the same number of DMAs per stage and the
// counted vmcnt waits stay exact.  The C tile leaves through LDS in passes of as many wave rows as fit the ring's bytes.
// block -> tile.  gx > 0: XCD (blockIdx % 8) owns the rectangle (xi, yi) of a gx x gy split of the tile grid (the panels it
// re-reads stay in its L2); gx == 0: XCD owns a contiguous run of ceil / floor(tiles / 8) tiles in M-fastest order (used
// when a rectangle split would put more than 32 tiles on one XCD although the grid fits the chip once).
__device__ __forceinline__ bool shaped_tile(int gx, int gy, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    if (gx == 0) {
        const int nwg = tiles_m * tiles_n, q = nwg >> 3, r = nwg & 7;
        if (local >= q + (xcd < r ? 1 : 0)) return false;
        const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
        tm = wgid % tiles_m;
        tn = wgid / tiles_m;
        return true;
    }
    const int xi = xcd % gx, yi = xcd / gx;
    const int qm = tiles_m / gx, rm = tiles_m % gx, qn = tiles_n / gy, rn = tiles_n % gy;
    const int m_begin = xi * qm + min(xi, rm), m_cnt = qm + (xi < rm ? 1 : 0);
    const int n_begin = yi * qn + min(yi, rn), n_cnt = qn + (yi < rn ? 1 : 0);
    if (m_cnt == 0 || local >= m_cnt * n_cnt) return false;
    tm = m_begin + local % m_cnt;
    tn = n_begin + local / m_cnt;
    return true;
}

// host side of shaped_tile: the split and the number of workgroups the fullest XCD receives
struct GridPlan { int gx, gy, per_xcd; };
inline GridPlan plan_grid(int tiles_m, int tiles_n, int bm, int bn) {
    GridPlan g{8, 1, 0};
    int best_cost = 1 << 30;
    const int cand[4] = {8, 4, 2, 1};
    for (int c = 0; c < 4; ++c) {
        const int gx = cand[c], gy = 8 / gx;
        const int cost = ((tiles_m + gx - 1) / gx) * bm + ((tiles_n + gy - 1) / gy) * bn;     // operand rows one XCD touches
        if (cost < best_cost) { best_cost = cost; g.gx = gx; g.gy = gy; }
    }
    g.per_xcd = ((tiles_m + g.gx - 1) / g.gx) * ((tiles_n + g.gy - 1) / g.gy);
    const int even = (tiles_m * tiles_n + 7) / 8;
    if ((g.per_xcd + 31) / 32 > (even + 31) / 32) { g.gx = 0; g.gy = 0; g.per_xcd = even; }
    return g;
}

template <int WM, int WN, int MF, int NF> struct TileGeo {
    static constexpr int NT = 64 * WM * WN, NW = WM * WN;
    static constexpr int TBM = 16 * MF * WM, TBN = 16 * NF * WN;
    static constexpr int AFULL = 4 * TBM / NT, BFULL = 4 * TBN / NT;
    static constexpr int BREM = (4 * TBN - BFULL * NT) / NW;             // lanes of the partial B piece per wave
    static constexpr int NDMA = AFULL + BFULL + (BREM > 0 ? 1 : 0);      // DMA instructions per wave and stage
    static constexpr int AOPER = TBM * 64, STAGE = (TBM + TBN) * 64, RING = 4 * STAGE;
    static constexpr int PITCH = TBN + 4;
    // wave rows staged per epilogue pass: the most that fit the ring
    static constexpr int SP = (16 * MF * WM * PITCH * 4 <= RING) ? WM : ((16 * MF * (WM / 2) * PITCH * 4 <= RING) ? WM / 2 : 1);
    static constexpr int PROWS = 16 * MF * SP;
    static constexpr int TPR = TBN / 4, RPP = NT / TPR, NPASS = (PROWS + RPP - 1) / RPP;
    static_assert(4 * TBM == AFULL * NT, "A stage must split evenly");
    static_assert(BFULL * NT + BREM * NW == 4 * TBN && BREM < 64, "B stage: full pieces + one partial piece per wave");
    static_assert(16 * MF * PITCH * 4 <= RING, "one wave row of C must fit the ring");
    static_assert(WM % SP == 0, "passes cover whole wave rows");
};

#define EAVQA_SHAPED_STEP(P, t)                                                                       \
    {                                                                                                 \
        const int rem = nk - 2 - (t);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        __builtin_amdgcn_s_waitcnt(0xC07F);       /* lgkmcnt(0): fragment set P is complete */         \
        if ((t) + 1 < nk) {                                                                           \
            if (rem >= 2) __builtin_amdgcn_s_waitcnt(vm_only(2 * G::NDMA));                           \
            else if (rem == 1) __builtin_amdgcn_s_waitcnt(vm_only(G::NDMA));                          \
            else __builtin_amdgcn_s_waitcnt(vm_only(0));                                              \
            __builtin_amdgcn_s_barrier();                                                             \
            if ((t) + 4 < nk) issue((t) + 4);                                                         \
            const char* st = smem + (((t) + 1) & 3) * G::STAGE;                                       \
            _Pragma("unroll") for (int i = 0; i < MF; ++i)                                            \
                fa[(P) ^ 1][i] = *reinterpret_cast<const bf16x8*>(st + a_off + i * 1024);             \
            _Pragma("unroll") for (int j = 0; j < NF; ++j)                                            \
                fb[(P) ^ 1][j] = *reinterpret_cast<const bf16x8*>(st + b_off + j * 1024);             \
        }                                                                                             \
        _Pragma("unroll") for (int i = 0; i < MF; ++i)                                                \
            _Pragma("unroll") for (int j = 0; j < NF; ++j)                                            \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[P][i], fb[P][j], acc[i][j], 0, 0, 0); \
    }

template <int WM, int WN, int MF, int NF>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN <= 4) ? 2 : 1) void gemm_bf16_shaped_kernel(GemmParams p, int gx, int gy, int tiles_m, int tiles_n) {
    using G = TileGeo<WM, WN, MF, NF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int tm, tn;
    if (!shaped_tile(gx, gy, tiles_m, tiles_n, tm, tn)) return;
    const int m0 = tm * G::TBM, n0 = tn * G::TBN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    // per-lane DMA sources; chunk c of an operand image is (row c >> 2, physical 16-byte slot c & 3)
    auto src_of = [&](const bf16_t* X, int64_t ld, int row0, int rows_max, int c) {
        const int row = c >> 2, pc = c & 3;
        return X + (int64_t)min(row0 + row, rows_max - 1) * ld + (pc ^ ((-(row >> 2)) & 3)) * 8;
    };
    const bf16_t* asrc[G::AFULL];
    const bf16_t* bsrc[G::BFULL + 1];
#pragma unroll
    for (int i = 0; i < G::AFULL; ++i) asrc[i] = src_of(A, p.lda, m0, p.M, tid + G::NT * i);
#pragma unroll
    for (int i = 0; i < G::BFULL; ++i) bsrc[i] = src_of(B, p.ldb, n0, p.N, tid + G::NT * i);
    bsrc[G::BFULL] = src_of(B, p.ldb, n0, p.N, G::BFULL * G::NT + wave * G::BREM + min(lane, max(G::BREM, 1) - 1));
    const int dma_off = wave * 1024;                                        // + i * NT * 16 for full pieces
    const int dma_off_x = G::AOPER + G::BFULL * G::NT * 16 + wave * G::BREM * 16;

    auto issue = [&](int kt) {
        char* st = smem + (kt & 3) * G::STAGE;
#pragma unroll
        for (int i = 0; i < G::AFULL; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off + i * G::NT * 16), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < G::BFULL; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + G::AOPER + dma_off + i * G::NT * 16), 16, 0, 0);
        if (G::BREM > 0 && lane < G::BREM)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[G::BFULL] + kt * FBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off_x), 16, 0, 0);
    };

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / FBK;
    const int frow = lane & 15, fk = lane >> 4;
    const int a_off = fswz(wm * 16 * MF + frow, fk);                   // + i * 16 rows * 64 B
    const int b_off = G::AOPER + fswz(wn * 16 * NF + frow, fk);        // + j * 16 rows * 64 B
    bf16x8 fa[2][MF], fb[2][NF];

#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < nk) issue(i);
    {
        const int later = min(nk, 4) - 1;
        if (later == 3) __builtin_amdgcn_s_waitcnt(vm_only(3 * G::NDMA));
        else if (later == 2) __builtin_amdgcn_s_waitcnt(vm_only(2 * G::NDMA));
        else if (later == 1) __builtin_amdgcn_s_waitcnt(vm_only(G::NDMA));
        else __builtin_amdgcn_s_waitcnt(vm_only(0));
    }
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < MF; ++i) fa[0][i] = *reinterpret_cast<const bf16x8*>(smem + a_off + i * 1024);
#pragma unroll
    for (int j = 0; j < NF; ++j) fb[0][j] = *reinterpret_cast<const bf16x8*>(smem + b_off + j * 1024);

    int t = 0;
    for (; t + 1 < nk; t += 2) {
        EAVQA_SHAPED_STEP(0, t)
        EAVQA_SHAPED_STEP(1, t + 1)
    }
    if (t < nk) EAVQA_SHAPED_STEP(0, t)
    __syncthreads();

    float* Cs = reinterpret_cast<float*>(smem);
    for (int pass = 0; pass < WM / G::SP; ++pass) {
        if (wm / G::SP == pass) {
            const int r0 = (wm % G::SP) * 16 * MF;
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = r0 + i * 16 + (lane >> 4) * 4 + r;
                        const int col = wn * 16 * NF + j * 16 + (lane & 15);
                        Cs[row * G::PITCH + col] = acc[i][j][r];
                    }
        }
        __syncthreads();
        epilogue<bf16_t, EpiGeo<G::TPR, G::RPP, G::NPASS, G::PITCH, G::PROWS>, false>(p, Cs, m0 + pass * G::PROWS, n0);
        if (pass + 1 < WM / G::SP) __syncthreads();
    }
}
#undef EAVQA_SHAPED_STEP

template <int WM, int WN, int MF, int NF>
int launch_shaped(const GemmParams& p, hipStream_t stream) {
    using G = TileGeo<WM, WN, MF, NF>;
    if (const int rc = opt_in_lds<gemm_bf16_shaped_kernel<WM, WN, MF, NF>>(G::RING)) return rc;
    const int tiles_m = (p.M + G::TBM - 1) / G::TBM, tiles_n = (p.N + G::TBN - 1) / G::TBN;
    const GridPlan g = plan_grid(tiles_m, tiles_n, G::TBM, G::TBN);
    hipLaunchKernelGGL((gemm_bf16_shaped_kernel<WM, WN, MF, NF>), dim3(g.per_xcd * 8), dim3(G::NT), G::RING, stream, p, g.gx, g.gy,
                       tiles_m, tiles_n);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}


// `rate`: measured ns per 64-byte operand row and K-step (32) of one workgroup alone on a CU (K = 5120 probes and the
// cfg2 shapes, tools/gemm_bench.py): the wider 8-wave tiles get closer to the MFMA / LDS limits and pay more per byte.
struct ShapeChoice { int bm, bn; float rate; int (*launch)(const GemmParams&, hipStream_t); };
const ShapeChoice SHAPES[5] = {
    {128, 80, 1.17f, launch_shaped<4, 1, 2, 5>}, {128, 96, 1.20f, launch_shaped<4, 1, 2, 6>},
    {256, 128, 1.15f, launch_shaped<4, 2, 4, 4>}, {256, 160, 1.23f, launch_shaped<4, 2, 4, 5>}, {256, 192, 1.39f, launch_shaped<4, 2, 4, 6>},
};
constexpr float RATE_FAST = 1.245f, RATE_BIG = 1.27f;

// Modelled time (ns, without the launch) of a grid of bm x bn tiles: the fullest XCD's workgroups per CU (co-resident
// ones share the CU's intake rate) x (operand bytes per K-step at that rate + the tile's epilogue).  Calibrated on MI355X
// (128 x 128: 17.8 us at K = 1280, 51.9 us at K = 5120; 256 x 128 on 240 tiles: 29 us at K = 1280).
inline float tile_cost(int M, int N, int K, int bm, int bn, float rate) {
    const int tiles_m = (M + bm - 1) / bm, tiles_n = (N + bn - 1) / bn;
    const GridPlan g = plan_grid(tiles_m, tiles_n, bm, bn);
    const float rounds = float((g.per_xcd + 31) / 32);
    return rounds * (rate * (bm + bn) * (K / 32) + 0.25f * bm * bn);
}

// ====================================================== bf16 big tiles ===
// 256 x 256 output tile per 1024-thread workgroup (16 waves as 4 x 4, 64 x 64 each, four waves per SIMD) for GEMMs
// with enough columns to give most CUs a tile (N >= 3840 on the hot path: QKV, FFN up, lm_head; the CLIP tower and
// the few-shot prefill).  Why: with 128 x 128 tiles every FLOP costs 1/64 B of L2 -> LDS traffic and the LDS-DMA path
// of a CU saturates near 30 B/clk, well before the matrix pipe; a 256 x 256 tile halves that (1/128 B per FLOP) and
// four waves per SIMD hide the fragment-read latency without a second register set.
//   * BK = 64: LDS rows are full 128-byte lines (every DMA instruction moves 8 whole rows), XOR swizzle chunk ^= row & 7;
//   * 2 stages x 64 KiB; tile t+1 is fetched (LDS-DMA) while tile t multiplies (32 MFMAs per wave ~ 2048 cycles per
//     SIMD, which covers an L2 round trip); one s_barrier per K-tile;
//   * the C tile leaves through LDS one 64-row slab at a time (the accumulators of one wave row).
constexpr int GBM = 256, GBN = 256, GBK = 64;
constexpr int BIG_GROUP_N = 8;                     // tile columns per group of the in-XCD order (tools/gemm_bench.py --group-n sweep, profiles/round3_tile_order.md)
constexpr int GOPER = GBM * GBK * 2;               // 32 KiB per operand per stage
constexpr int GSTAGE = 2 * GOPER;                  // 64 KiB
constexpr int GCS_PITCH = GBN + 4;                 // floats per staged C row
constexpr int GLDS_BYTES = 2 * GSTAGE;             // 128 KiB (the 64 x 260 fp32 slab reuses it)
using EpiGeo256 = EpiGeo<64, 16, 4, GCS_PITCH, 64, 1>;    // 64 x 256 slab, 1024 threads (128 registers per lane: one pass at a time in the eavqa_gemm_ln form)

// Order of an XCD's tiles in time (its 32 CUs take them in `local` order): column groups of GN tile columns, inside a group n
// fastest.  The 32 tiles in flight are then 32 / GN tile rows x GN columns: every A panel is shared by GN concurrent tiles and the
// group's GN B panels stay in the XCD's L2 while the rows stream by - with m fastest (round 2) a multi-round problem re-read
// every A panel once per tile column from beyond L2 (FFN-down of the CLIP tower: 4 columns -> the 337 MB A operand four times).
__device__ __forceinline__ bool big_tile(const GemmParams& p, int gx, int gy, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int xi = xcd % gx, yi = xcd / gx;
    const int qm = tiles_m / gx, rm = tiles_m % gx, qn = tiles_n / gy, rn = tiles_n % gy;
    const int m_begin = xi * qm + min(xi, rm), m_cnt = qm + (xi < rm ? 1 : 0);
    const int n_begin = yi * qn + min(yi, rn), n_cnt = qn + (yi < rn ? 1 : 0);
    if (m_cnt == 0 || local >= m_cnt * n_cnt) return false;
    const int GN = p.group_n;
    if (GN <= 0) {                                     // m fastest (round 2 order; one-round problems do not care)
        tm = m_begin + local % m_cnt;
        tn = n_begin + local / m_cnt;
        return true;
    }
    const int per_group = m_cnt * GN;
    const int g = local / per_group, r = local - g * per_group;
    const int gn = min(GN, n_cnt - g * GN);           // columns of this (possibly last, narrower) group
    tm = m_begin + r / gn;
    tn = n_begin + g * GN + r % gn;
    return true;
}

template <bool LNX>
__global__ __launch_bounds__(1024) void gemm_bf16_big_kernel(typename KernArg<LNX>::type pk, int gx, int gy, int tiles_m, int tiles_n) {
    const GemmParams p = widen(pk);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int tm, tn;
    if (!big_tile(p, gx, gy, tiles_m, tiles_n, tm, tn)) return;
    const int m0 = tm * GBM, n0 = tn * GBN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const bf16_t* A = reinterpret_cast<const bf16_t*>(p.A);
    const bf16_t* B = reinterpret_cast<const bf16_t*>(p.B);

    // DMA sources: chunk c = tid + 1024 i of the [256 rows][8 chunks] image (row = c >> 3, physical chunk c & 7)
    const bf16_t* asrc[2];
    const bf16_t* bsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 1024 * i;
        const int row = c >> 3, pc = c & 7;
        asrc[i] = A + (int64_t)min(m0 + row, p.M - 1) * p.lda + (pc ^ (row & 7)) * 8;
        bsrc[i] = B + (int64_t)min(n0 + row, p.N - 1) * p.ldb + (pc ^ (row & 7)) * 8;
    }
    const int dma_off = wave * 1024;
    auto issue = [&](int kt) {
        char* st = smem + (kt & 1) * GSTAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + kt * GBK),
                                             (__attribute__((address_space(3))) void*)(st + dma_off + i * 16384), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + kt * GBK),
                                             (__attribute__((address_space(3))) void*)(st + GOPER + dma_off + i * 16384), 16, 0, 0);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / GBK;
    const int frow = lane & 15, fk = lane >> 4;
    const int arow = wm * 64 + frow, brow = wn * 64 + frow;     // + 16 i ; row & 7 == frow & 7 for every fragment
    issue(0);
    float2* rowstat = reinterpret_cast<float2*>(smem + GLDS_BYTES);     // eavqa_gemm_ln: under the first tile's round trip
    if (LNX) ln_rowstat_fill(p, rowstat, m0, n0, GBM, tid, 1024);
    for (int kt = 0; kt < nk; ++kt) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0070);        // vmcnt(0) lgkmcnt(0): this wave's share of tile kt has landed
        __builtin_amdgcn_s_barrier();              // ... and everybody's; all reads of the other stage are done
        if (kt + 1 < nk) issue(kt + 1);
        const char* st = smem + (kt & 1) * GSTAGE;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 af[4], bfr[4];
            const int sw = ((s * 4 + fk) ^ (frow & 7)) << 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8*>(st + (arow + 16 * i) * 128 + sw);
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(st + GOPER + (brow + 16 * j) * 128 + sw);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();

    float* Cs = reinterpret_cast<float*>(smem);
    for (int slab = 0; slab < 4; ++slab) {
        if (wm == slab) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = i * 16 + (lane >> 4) * 4 + r;
                        const int col = wn * 64 + j * 16 + (lane & 15);
                        Cs[row * GCS_PITCH + col] = acc[i][j][r];
                    }
        }
        __syncthreads();
        epilogue<bf16_t, EpiGeo256, LNX>(p, Cs, m0 + slab * 64, n0, LnArgs{rowstat, slab * 64});
        __syncthreads();
    }
}

// XCD rectangle of the 256 x 256 kernel: gx x gy XCDs over tile rows x tile columns with the fewest panels per XCD; returns tiles per XCD
// (round 3: fewest ROUNDS of 32 workgroups per XCD first - the few-shot prefill's FFN-up, 19 x 40 tiles, is 10 x 10 = 100 tiles per XCD =
// four rounds on the 2 x 4 rectangle with the fewest panels but 19 x 5 = 95 = three rounds on 1 x 8 - then the fewest panels)
inline int big_grid(int tiles_m, int tiles_n, int& gx, int& gy) {
    int best_gx = 8, best_cost = 1 << 30, best_rounds = 1 << 30;
    const int cand[4] = {8, 4, 2, 1};
    for (int c = 0; c < 4; ++c) {
        const int x = cand[c], y = 8 / x;
        const int pm = (tiles_m + x - 1) / x, pn = (tiles_n + y - 1) / y;
        const int rounds = (pm * pn + 31) / 32, cost = pm + pn;
        if (rounds < best_rounds || (rounds == best_rounds && cost < best_cost)) { best_rounds = rounds; best_cost = cost; best_gx = x; }
    }
    gx = best_gx; gy = 8 / gx;
    return ((tiles_m + gx - 1) / gx) * ((tiles_n + gy - 1) / gy);
}

int launch_big(const GemmParams& p, hipStream_t stream) {
    const int tiles_m = (p.M + GBM - 1) / GBM, tiles_n = (p.N + GBN - 1) / GBN;
    int gx, gy;
    const int per_xcd = big_grid(tiles_m, tiles_n, gx, gy);
    if (p.ln_stats || p.stats_out || p.copy_out) {      // eavqa_gemm_ln: its own instantiation (the plain one has no registers to spare)
        if (const int rc = opt_in_lds<gemm_bf16_big_kernel<true>>(GLDS_BYTES + LN_ROWSTAT_BYTES)) return rc;
        hipLaunchKernelGGL(gemm_bf16_big_kernel<true>, dim3(per_xcd * 8), dim3(1024), GLDS_BYTES + ln_lds(p), stream, p, gx, gy, tiles_m, tiles_n);
    } else {
        if (const int rc = opt_in_lds<gemm_bf16_big_kernel<false>>(GLDS_BYTES)) return rc;
        hipLaunchKernelGGL(gemm_bf16_big_kernel<false>, dim3(per_xcd * 8), dim3(1024), GLDS_BYTES, stream, p, gx, gy, tiles_m, tiles_n);
    }
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

// Rows to hand to a second, small-tile launch (0 = none): when the last tile row is ragged (M % 256 <= 192 rows) and the problem without it
// needs one round of workgroups less.  The CLIP tower at 64 images is M = 16 448 = 64 tile rows + 64 rows: out-proj / FFN-down are 260
// tiles = TWO rounds for 256 CUs (the second one of four tiles), QKV 780 = four rounds instead of three; at 160 images FFN-up is 2 576
// tiles = eleven rounds instead of ten.  Every tile costs the same whatever its valid rows, so the few ragged rows cost a whole round.
inline int big_split_rows(int M, int N) {
    const int rem = M % GBM;
    if (rem == 0 || rem > 192 || M <= GBM) return 0;
    int gx, gy;
    const int tiles_n = (N + GBN - 1) / GBN;
    const int with = (big_grid((M + GBM - 1) / GBM, tiles_n, gx, gy) + 31) / 32, without = (big_grid(M / GBM, tiles_n, gx, gy) + 31) / 32;
    return without < with ? rem : 0;
}

bool use_big(int M, int N, int K, const Knobs& kn) {
    if (K % GBK) return false;
    if (kn.big_mode == 1) return false;
    if (kn.big_mode == 2) return true;
    const int tiles = ((M + GBM - 1) / GBM) * ((N + GBN - 1) / GBN);
    return tiles >= 144;     // measured crossover on MI355X: below ~140 tiles the 128 x 128 kernel (more CUs busy) wins
}
