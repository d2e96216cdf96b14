// Decode attention (Sq = 1, bf16): the kernel, its domain (decode_supported), the table of its variants and its launcher; which variant a
// shape gets is decode_plan (decode_params.h).  Included by attention.hip (same translation unit), whose forward dispatcher tries it first.
#include "attention_params.h"
#include "decode_params.h"

namespace {

// One new query per sample against a cache of Sk keys: the work is reading K and V once, and at decode batch sizes the
// kernel is a chain of dependent HBM round trips (measured 19.7 us at B = 8 and 23.3 us at B = 32 with one wave walking
// all keys of a head: latency, not bytes).  So the walk is cut short instead: a workgroup = 4 neighbouring heads of one
// sample (their K / V slices are adjacent in the [S, E] cache rows) x DEC_WPH waves per head, each wave taking every
// DEC_WPH-th group of keys; a wave gives LPK lanes to a key (16 bytes = 8 head dims each) and walks 64 / LPK keys per load
// instruction, DEC_U instructions in flight - 160 keys are ONE batch of loads per wave for K and one for V.  Scores go
// to LDS; every wave of a head reduces max / sum over all of them itself (no second exchange); the partial outputs of the
// DEC_WPH waves are summed through LDS in wave order.  Same masking rule as the tiled kernels: masked scores become
// -FLT_MAX (a fully masked row averages all keys).
// DEC_WPH: 4 when the grid fits the chip once (one 16-wave workgroup per CU), fewer for larger batches, where several smaller
// workgroups per CU overlap their latency chains instead.
// VLDS: V does not depend on the scores, so its bytes should be on their way while K is being scored - but a second batch of loads
// held in registers does not fit a 16-wave workgroup's 128 VGPRs (measured: 41 spilled registers, 26.5 us against 18 us).  So the
// whole V slice of the workgroup ([Sk keys][4 heads x hd], 100 KiB at Sk = 160, hd = 80) is fetched by LDS-DMA at the very start,
// costs no registers, and P.V reads it from LDS: the kernel is ONE HBM round trip.  Taken when the image fits (<= 128 KiB) and
// the grid is one workgroup per CU.
// Phase timestamps of workgroup (0, 0), one row per wave: only in the profiling build (tools/attn_stamps.sh, -DEAVQA_ATTN_STAMPS); the
// shipped library compiles EAVQA_STAMP to nothing.
#ifdef EAVQA_ATTN_STAMPS
__device__ unsigned long long eavqa_attn_stamps[16 * 16];
#define EAVQA_STAMP(i) do { if (blockIdx.x == 0 && blockIdx.y == 0 && (threadIdx.x & 63) == 0) eavqa_attn_stamps[(threadIdx.x >> 6) * 16 + (i)] = wall_clock64(); } while (0)
#else
#define EAVQA_STAMP(i) do { } while (0)
#endif

// what the kernel is told (the fields are explained at its head)
struct DecodeArgs {
    const bf16_t* q; int64_t ldq; const bf16_t* k; int64_t ldk; const bf16_t* v; int64_t ldv; bf16_t* out; int64_t ldo; int64_t bsq, bsk;
    const int32_t* key_mask; int64_t ld_mask; float* lse; int H, Sk, hd; float scale;
    const bf16_t* k_new; const bf16_t* v_new; int64_t ld_new; const float* qkv_part; int ks; const float* qkv_bias; int part_cols, part_kv;
    const float* rel_bias; int64_t rel_ld; int rel_zero;
};

// VMODE 2 (round 4): BOTH batches in registers and in flight from the first instruction on - K, then V - on workgroups of 4 heads x 1 or 2
// waves (at most 8 waves per CU: 256 VGPRs each, room for 2 x DEC_U x 4 data registers).  tools/attn_stamps.py showed where the LDS-image
// kernel's 20 us go: ISSUING the ~100 LDS-DMA instructions of a CU takes 4.3 us for its first wave and 9.6 us for its sixteenth (an LDS-DMA
// holds the CU's issue for ~40 ns), the K loads queue behind them, and every wave then waits at the barrier for the last one's scores
// (15.4 us).  Plain loads issue in ~1 us and the kernel is one HBM round trip.  DEC_WPH == 1 (a head's keys fit one wave's batch: T5's
// decoder self-attention, <= 80 keys) also drops the cross-wave exchange of partial outputs and its barrier.
template <int LPK, int DEC_WPH, int DEC_U, int VMODE>
__global__ __launch_bounds__(256 * DEC_WPH) void attn_decode_kernel(DecodeArgs args) {
    // k_new / v_new (eavqa_attention_decode): the K / V rows of the NEW position (key Sk - 1) still sit in the QKV projection's
    // output; the lanes that own that key take them from there and append them to the cache on the way (each 16-byte piece of a
    // cache row has exactly one owner lane), which saves the separate append pass of the decode step.
    // qkv_part (eavqa_attention_decode_splitk): q and the new K / V rows do not exist yet - the QKV projection left `ks` fp32 partial
    // sums [ks][B][3 E]; every lane adds up the 8 values it needs (slices in index order, then the bias, then rounded to bf16: exactly
    // what eavqa_splitk_finish would have stored), which also saves the finish pass.  part_cols = columns per row of the partial sums
    // (3 H hd: q | k | v, part_kv != 0; H hd: a cross-attention's q alone, part_kv == 0 - nothing to append).
    // rel_bias (T5, HF:t5 :217-279): score(j) += rel_bias[h * rel_ld + (j - (Sk - 1)) + rel_zero] - the one query sits at position Sk - 1.
    const bf16_t* __restrict__ q = args.q; const bf16_t* __restrict__ k = args.k; const bf16_t* __restrict__ v = args.v; bf16_t* __restrict__ out = args.out;
    const int64_t ldq = args.ldq, ldk = args.ldk, ldv = args.ldv, ldo = args.ldo, bsq = args.bsq, bsk = args.bsk, ld_mask = args.ld_mask, ld_new = args.ld_new, rel_ld = args.rel_ld;
    const int32_t* __restrict__ key_mask = args.key_mask; float* __restrict__ lse = args.lse;
    const int H = args.H, Sk = args.Sk, hd = args.hd, ks = args.ks, part_cols = args.part_cols, part_kv = args.part_kv, rel_zero = args.rel_zero; const float scale = args.scale;
    const bf16_t* __restrict__ k_new = args.k_new; const bf16_t* __restrict__ v_new = args.v_new;
    const float* __restrict__ qkv_part = args.qkv_part; const float* __restrict__ qkv_bias = args.qkv_bias; const float* __restrict__ rel_bias = args.rel_bias;
    extern __shared__ float dec_sc[];                 // [4 heads][Sk] scores, then [4][DEC_WPH][128] partial outputs, then the V image
    EAVQA_STAMP(0);
    constexpr bool VLDS = VMODE == 1, VREG = VMODE == 2;
    constexpr int KPI = 64 / LPK;
    char* vimg = reinterpret_cast<char*>(dec_sc + 4 * Sk + 4 * DEC_WPH * 128);      // VLDS: [Sk][4 heads x hd] bf16
    const int cpk = hd >> 1;                          // 16-byte pieces per key in the image (4 heads x hd / 8)
    const bool appended = (qkv_part && part_kv) || k_new;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hh = wave / DEC_WPH, part = wave % DEC_WPH;
    const int b = blockIdx.x, h = blockIdx.y * 4 + hh;
    const bool head_ok = h < H;
    const int sub = lane / LPK, dl = lane % LPK;
    const bool active = head_ok && 8 * dl < hd;
    float* sc = dec_sc + hh * Sk;
    float* opart = dec_sc + 4 * Sk + (hh * DEC_WPH + part) * 128;
    constexpr int STEP = KPI * DEC_WPH * DEC_U;
    const int E3 = part_cols;
    // bf16(sum_s P[s][b][col .. col+7] + bias[col ..]) - the value eavqa_splitk_finish stores
    auto from_part = [&](int col) -> bf16x8 {
        const float* p0 = qkv_part + (int64_t)b * E3 + col;
        const int64_t slice = (int64_t)gridDim.x * E3;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
        for (int s0 = 0; s0 < ks; s0 += 4) {              // four slices' loads in flight, added in index order
            float4 ta[4], tc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* ps = p0 + min(s0 + i, ks - 1) * slice;
                ta[i] = *reinterpret_cast<const float4*>(ps);
                tc[i] = *reinterpret_cast<const float4*>(ps + 4);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (s0 + i == 0) { a = ta[0]; c = tc[0]; }
                else if (s0 + i < ks) {
                    a.x += ta[i].x; a.y += ta[i].y; a.z += ta[i].z; a.w += ta[i].w;
                    c.x += tc[i].x; c.y += tc[i].y; c.z += tc[i].z; c.w += tc[i].w;
                }
            }
        }
        if (qkv_bias) {
            const float4 a2 = *reinterpret_cast<const float4*>(qkv_bias + col), c2 = *reinterpret_cast<const float4*>(qkv_bias + col + 4);
            a.x += a2.x; a.y += a2.y; a.z += a2.z; a.w += a2.w; c.x += c2.x; c.y += c2.y; c.z += c2.z; c.w += c2.w;
        }
        bf16x8 r;
        r[0] = (bf16_t)a.x; r[1] = (bf16_t)a.y; r[2] = (bf16_t)a.z; r[3] = (bf16_t)a.w;
        r[4] = (bf16_t)c.x; r[5] = (bf16_t)c.y; r[6] = (bf16_t)c.z; r[7] = (bf16_t)c.w;
        return r;
    };
    const bf16_t* kb = k + (int64_t)b * bsk * ldk + h * hd + 8 * dl;
    const bf16_t* vb = v + (int64_t)b * bsk * ldv + h * hd + 8 * dl;
    if (VLDS) {
        const int n_keys = appended ? Sk - 1 : Sk;    // the new key's row is not in the cache yet: its owner lanes write the image
        const int total = n_keys * cpk;
        const int valid_pieces = min(cpk, ((H - blockIdx.y * 4) * hd) >> 3);      // a last group of < 4 heads: stay inside the row
        const bf16_t* vsrc = v + (int64_t)b * bsk * ldv + blockIdx.y * 4 * hd;
        for (int base = __builtin_amdgcn_readfirstlane(wave) * 64; base < total; base += 64 * 4 * DEC_WPH) {
            const int c = base + lane;
            const int key = c / cpk, piece = c - key * cpk;
            if (c < total && piece < valid_pieces)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vsrc + (int64_t)key * ldv + piece * 8),
                                                 (__attribute__((address_space(3))) void*)(vimg + base * 16), 16, 0, 0);
        }
    }
    // key of (batch start j0, slot u): groups of KPI keys are dealt round-robin to the DEC_WPH waves of the head
    auto key_of = [&](int j0, int u) { return j0 + (u * DEC_WPH + part) * KPI + sub; };
    // the first batch of K goes out before anything that has to wait for the previous kernel's results (q and the new K / V row
    // below): those L2 round trips then run under the HBM round trip instead of in front of it
    bf16x8 kv0[DEC_U];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
        const int j = key_of(0, u);
        kv0[u] = (bf16x8){};
        if (active && j < Sk) kv0[u] = *reinterpret_cast<const bf16x8*>(kb + (int64_t)j * ldk);    // row Sk-1 may be stale: patched below
    }
    bf16x8 vpre[VREG ? DEC_U : 1];                    // VMODE 2: the first batch of V right behind it (same patch for row Sk-1)
    if (VREG) {
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int j = key_of(0, u);
            vpre[u] = (bf16x8){};
            if (active && j < Sk) vpre[u] = *reinterpret_cast<const bf16x8*>(vb + (int64_t)j * ldv);
        }
    }
    EAVQA_STAMP(1);
    // the new position: its one owner lane per 16-byte piece fetches (or sums up) the row and appends it to the cache
    bf16x8 knew = {}, vnew = {};
    bool own_new = false;
    if (appended) {
        const int rem = (Sk - 1) % STEP, grp = rem / KPI;
        own_new = active && (rem % KPI) == sub && (grp % DEC_WPH) == part;
        if (own_new) {
            if (qkv_part) {
                knew = from_part(H * hd + h * hd + 8 * dl);
                vnew = from_part(2 * H * hd + h * hd + 8 * dl);
            } else {
                knew = *reinterpret_cast<const bf16x8*>(k_new + (int64_t)b * ld_new + h * hd + 8 * dl);
                vnew = *reinterpret_cast<const bf16x8*>(v_new + (int64_t)b * ld_new + h * hd + 8 * dl);
            }
            *reinterpret_cast<bf16x8*>(const_cast<bf16_t*>(kb) + (int64_t)(Sk - 1) * ldk) = knew;
            *reinterpret_cast<bf16x8*>(const_cast<bf16_t*>(vb) + (int64_t)(Sk - 1) * ldv) = vnew;
            if (VLDS) *reinterpret_cast<bf16x8*>(vimg + ((Sk - 1) * cpk + hh * (hd >> 3) + dl) * 16) = vnew;
        }
    }
    EAVQA_STAMP(2);
    float qf[8];
    {
        bf16x8 t = {};
        if (active) t = qkv_part ? from_part(h * hd + 8 * dl) : *reinterpret_cast<const bf16x8*>(q + (int64_t)b * bsq * ldq + h * hd + 8 * dl);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = (float)t[e];
    }
    auto load_k = [&](int j) -> bf16x8 {
        if (own_new && j == Sk - 1) return knew;
        return *reinterpret_cast<const bf16x8*>(kb + (int64_t)j * ldk);
    };
    auto load_v = [&](int j) -> bf16x8 {
        if (own_new && j == Sk - 1) return vnew;
        return *reinterpret_cast<const bf16x8*>(vb + (int64_t)j * ldv);
    };
    const int32_t* mrow = key_mask ? key_mask + (int64_t)b * ld_mask : nullptr;
    EAVQA_STAMP(3);

    auto score = [&](const bf16x8 (&kv)[DEC_U], int j0) {
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int j = key_of(j0, u);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d += qf[e] * (float)kv[u][e];
#pragma unroll
            for (int o = LPK >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
            if (head_ok && dl == 0 && j < Sk)
                sc[j] = (mrow && mrow[j] == 0) ? -FLT_MAX : d * scale + (rel_bias ? rel_bias[(int64_t)h * rel_ld + (j - (Sk - 1)) + rel_zero] : 0.f);
        }
    };
    // first batch: the registers loaded at kernel start, the stale new row patched in place (no copy: with 2 x 20 loads held a second
    // set of K registers spilled 137 VGPRs)
#pragma unroll
    for (int u = 0; u < DEC_U; ++u)
        if (own_new && key_of(0, u) == Sk - 1) kv0[u] = knew;
    score(kv0, 0);
    for (int j0 = STEP; j0 < Sk; j0 += STEP) {
        bf16x8 kv[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int j = key_of(j0, u);
            kv[u] = (bf16x8){};
            if (active && j < Sk) kv[u] = load_k(j);
        }
        score(kv, j0);
    }
    EAVQA_STAMP(4);
    // without the image, the first batch of V is fetched under the exchange and the softmax
    bf16x8 v0[VMODE == 0 ? DEC_U : 1];
    if (VMODE == 0) {
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int j = key_of(0, u);
            v0[u] = (bf16x8){};
            if (active && j < Sk) v0[u] = load_v(j);
        }
    } else if (VLDS) {
        __builtin_amdgcn_s_waitcnt(0x0070 | 0x0F00);      // vmcnt(0): this wave's share of the V image has landed
    }
    EAVQA_STAMP(5);
    __syncthreads();
    EAVQA_STAMP(6);
    float mx = -FLT_MAX;
    for (int j = lane; j < Sk; j += 64) mx = fmaxf(mx, sc[j]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < Sk; j += 64) sum += __expf(sc[j] - mx);
    sum = wave_sum(sum);

    EAVQA_STAMP(7);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto accumulate = [&](const bf16x8 (&vv)[DEC_U], int j0) {
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int j = key_of(j0, u);
            const float pj = (active && j < Sk) ? __expf(sc[j] - mx) : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += pj * (float)vv[u][e];
        }
    };
    if (VMODE == 0) accumulate(reinterpret_cast<const bf16x8 (&)[DEC_U]>(v0), 0);
    if (VREG) {
#pragma unroll
        for (int u = 0; u < DEC_U; ++u)
            if (own_new && key_of(0, u) == Sk - 1) vpre[u] = vnew;
        accumulate(reinterpret_cast<const bf16x8 (&)[DEC_U]>(vpre), 0);
    }
    for (int j0 = VLDS ? 0 : STEP; j0 < Sk; j0 += STEP) {
        bf16x8 vv[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int j = key_of(j0, u);
            vv[u] = (bf16x8){};
            if (active && j < Sk)
                vv[u] = VLDS ? *reinterpret_cast<const bf16x8*>(vimg + (j * cpk + hh * (hd >> 3) + dl) * 16) : load_v(j);
        }
        accumulate(vv, j0);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int off = LPK; off < 64; off <<= 1) o[e] += __shfl_xor(o[e], off, 64);
    EAVQA_STAMP(8);
    if (DEC_WPH == 1) {                               // the wave holds its head's whole output: no exchange
        if (sub == 0 && active) {
            const float inv = 1.f / sum;
            bf16x8 r;
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (bf16_t)(o[e] * inv);
            *reinterpret_cast<bf16x8*>(out + (int64_t)b * bsq * ldo + h * hd + 8 * dl) = r;
        }
        if (lse && head_ok && lane == 0) lse[(int64_t)b * H + h] = mx + __logf(sum);
        EAVQA_STAMP(9);
        return;
    }
    __syncthreads();                                  // every wave is done reading the scores: reuse nothing of theirs
    if (sub == 0 && active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) opart[8 * dl + e] = o[e];
    }
    __syncthreads();
    if (part == 0 && sub == 0 && active) {
        const float* p0 = dec_sc + 4 * Sk + hh * DEC_WPH * 128 + 8 * dl;
        const float inv = 1.f / sum;
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = p0[e];
#pragma unroll
            for (int w = 1; w < DEC_WPH; ++w) t += p0[w * 128 + e];
            r[e] = (bf16_t)(t * inv);
        }
        *reinterpret_cast<bf16x8*>(out + (int64_t)b * bsq * ldo + h * hd + 8 * dl) = r;
    }
    if (lse && head_ok && part == 0 && lane == 0) lse[(int64_t)b * H + h] = mx + __logf(sum);
    EAVQA_STAMP(9);
}

bool decode_supported(const AttnCall& c) {
    const AttnParams& p = c.p;
    return c.dtype == EAVQA_BF16 && p.Sq == 1 && !p.cu && p.hd % 8 == 0 && p.hd <= 128 && p.Sk <= 3584 && (p.ldq % 8 == 0) && (p.ldk % 8 == 0) &&
           (p.ldv % 8 == 0) && (p.ldo % 8 == 0);
}

DecodePlan decode_plan(const AttnCall& c) { return decode_plan(c.p.B, c.p.H, c.p.Sk, c.p.hd, c.path); }

// f(kernel) for the plan's variant; every instantiated variant is in this table: (lanes per key, waves per head, loads in flight, V mode)
template <typename F> bool with_decode_kernel(const DecodePlan& p, F&& f) {
    return with_value<8, 16>(p.lpk, [&](auto LPK) {
        auto row = [&](auto WPH, auto U, auto VM) {
            constexpr int lpk = decltype(LPK)::value, wph = decltype(WPH)::value, u = decltype(U)::value, vm = decltype(VM)::value;
            return p.wph == wph && p.u == u && p.vmode == vm && (f(KernelTag<attn_decode_kernel<lpk, wph, u, vm>>{}), true);
        };
        return row(Int<1>{}, Int<10>{}, Int<2>{}) || row(Int<2>{}, Int<10>{}, Int<2>{}) || row(Int<2>{}, Int<20>{}, Int<2>{}) ||
               row(Int<4>{}, Int<10>{}, Int<1>{}) ||
               row(Int<4>{}, Int<10>{}, Int<0>{}) || row(Int<2>{}, Int<10>{}, Int<0>{}) || row(Int<1>{}, Int<10>{}, Int<0>{});
    });
}

DecodeArgs decode_args(const AttnCall& c) {
    const AttnParams& p = c.p;
    const int H = p.H, Sk = p.Sk, hd = p.hd;
    DecodeArgs a = {};
    a.q = reinterpret_cast<const bf16_t*>(p.q); a.k = reinterpret_cast<const bf16_t*>(p.k); a.v = reinterpret_cast<const bf16_t*>(p.v);
    a.out = reinterpret_cast<bf16_t*>(p.out); a.ldq = p.ldq; a.ldk = p.ldk; a.ldv = p.ldv; a.ldo = p.ldo; a.bsq = p.bsq; a.bsk = p.bsk;
    a.key_mask = p.key_mask; a.ld_mask = p.ld_mask; a.lse = p.lse; a.H = H; a.Sk = Sk; a.hd = hd; a.scale = p.scale;
    a.k_new = reinterpret_cast<const bf16_t*>(c.k_new); a.v_new = reinterpret_cast<const bf16_t*>(c.v_new); a.ld_new = c.ld_new;
    a.qkv_part = c.qkv_part; a.ks = c.ks; a.qkv_bias = c.qkv_bias; a.rel_bias = p.rel_bias; a.rel_ld = p.rel_ld; a.rel_zero = p.rel_zero;
    a.part_cols = c.part_cols ? c.part_cols : 3 * H * hd;               // columns per row of the partial sums; q | k | v unless told otherwise
    a.part_kv = c.part_cols == 0 || c.part_cols == 3 * H * hd;
    return a;
}

// plan, opt in (the LDS image alone asks for more than the default limit), fill args, launch; attention_forward has validated the call
int launch_decode(const AttnCall& c) {
    const DecodePlan p = decode_plan(c);
    int rc = EAVQA_E_SHAPE;                                 // (no such variant: the plan and the table disagree)
    with_decode_kernel(p, [&](auto k) {
        constexpr auto kernel = decltype(k)::value;
        if (p.vmode == 1 && (rc = opt_in_lds<kernel>(DECODE_LDS_MAX))) return;
        hipLaunchKernelGGL(kernel, p.grid, dim3(p.block), p.lds, c.stream, decode_args(c));
        rc = hipGetLastError() != hipSuccess ? EAVQA_E_LAUNCH : EAVQA_OK;
    });
    return rc;
}

}  // namespace
