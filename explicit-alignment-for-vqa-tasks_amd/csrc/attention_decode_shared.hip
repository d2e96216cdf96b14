// Decode attention for G rows per prompt (beams or draws) over ONE shared prompt K / V cache: eavqa_attention_decode_shared.
// Its own translation unit (build.py HIP_SOURCES); bf16 and fp32 storage, fp32 arithmetic.
#include "common.h"

namespace {

// Row (b, g) attends [prompt b's S0 cached keys, masked by key_mask | its own tail positions 0..t].  Replicating the prompt per beam
// makes a step read G times the prompt bytes; here a workgroup = 4 neighbouring heads of ONE prompt x SH_WPH waves per head serves all G
// queries: every prompt K / V piece a lane loads is scored against, and accumulated into, all G rows before the next one is fetched.
// What attention_decode.hip measured holds here too (latency, not bytes): a lane takes 16 bytes of a key, a wave walks 64 / LPK keys per
// load instruction, SH_U instructions of K AND of V are in flight together (plain loads, V does not wait for the scores).
// G queries' scores over up to 3584 + 256 keys do not fit LDS (8 x 4 heads x 3840 floats), so the softmax runs online: every wave keeps
// (running max, sum, fp32 output) per row in registers, rescaled once per batch, and the SH_WPH waves of a head are merged through LDS
// by their maxima at the end - one rounding to the storage type.  A masked prompt key has weight exactly 0 (it enters neither the max
// nor the sum); tail key t is never masked, so every row has at least one key.
// Tail: slot u of a batch belongs to row u % G, so each row's own keys take the same lanes, in the same order, as every other row's -
// rows of one prompt with equal q and equal tails come out bit-identical.  The lanes that own tail position t take it from k_new / v_new
// and append it to the tail cache on the way (each 16-byte piece has exactly one owner), as eavqa_attention_decode does.
// Bit-identical twins need every row's arithmetic to be the SAME instructions: the loops over rows are unrolled, and the compiler may
// contract a multiply-add into an fma in one copy and not in another (measured: fp32 twins differed in the last bit).  So contraction is
// off in this file and the multiply-adds that should fuse say so themselves.
#pragma clang fp contract(off)
constexpr int SH_WPH = 2, SH_U = 8, SH_GMAX = 8;

template <typename T> struct Piece;                    // 16 bytes of storage type T
template <> struct Piece<bf16_t> { typedef bf16x8 vec; static constexpr int N = 8; };
template <> struct Piece<float> { typedef f32x4 vec; static constexpr int N = 4; };

struct SharedArgs {
    const void* q; int64_t ldq; const void* kp; int64_t ldk; const void* vp; int64_t ldv; int64_t pbr;
    void* kt; void* vt; int64_t ldt; const void* k_new; const void* v_new; int64_t ld_new; void* out; int64_t ldo;
    const int32_t* key_mask; int64_t ld_mask; int G, H, S0, t, t_max, hd; float scale;
};

template <typename T, int LPK>
__global__ __launch_bounds__(256 * SH_WPH) void attn_decode_shared_kernel(SharedArgs a) {
    typedef typename Piece<T>::vec vec_t;
    constexpr int EPL = Piece<T>::N;                   // elements per lane
    constexpr int KPI = 64 / LPK;                      // keys per load instruction
    constexpr int STEP = KPI * SH_WPH * SH_U;          // prompt keys per batch of a head
    __shared__ float qs[4][SH_GMAX][128];              // the G queries of the 4 heads, fp32
    __shared__ float comb_o[4][SH_WPH][SH_GMAX][128];  // per-wave partial outputs
    __shared__ float comb_m[4][SH_WPH][SH_GMAX], comb_l[4][SH_WPH][SH_GMAX];
    const int G = a.G, H = a.H, S0 = a.S0, t = a.t, hd = a.hd;
    const float scale = a.scale;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hh = wave / SH_WPH, part = wave % SH_WPH;
    const int b = blockIdx.x, h = blockIdx.y * 4 + hh;
    const bool head_ok = h < H;
    const int sub = lane / LPK, dl = lane % LPK;
    const bool active = head_ok && EPL * dl < hd;
    const int col = h * hd + EPL * dl;
    const T* kp = static_cast<const T*>(a.kp) + (int64_t)b * a.pbr * a.ldk + col;
    const T* vp = static_cast<const T*>(a.vp) + (int64_t)b * a.pbr * a.ldv + col;
    const int32_t* mrow = a.key_mask ? a.key_mask + (int64_t)b * a.ld_mask : nullptr;

    vec_t kr[SH_U], vr[SH_U];
    unsigned att = 0;                                  // bit u: slot u holds an attended key of this lane
    auto load_prompt = [&](int j0) {
        att = 0;
#pragma unroll
        for (int u = 0; u < SH_U; ++u) {
            const int j = j0 + (u * SH_WPH + part) * KPI + sub;
            kr[u] = (vec_t){}; vr[u] = (vec_t){};
            if (active && j < S0) {
                kr[u] = *reinterpret_cast<const vec_t*>(kp + (int64_t)j * a.ldk);
                vr[u] = *reinterpret_cast<const vec_t*>(vp + (int64_t)j * a.ldv);
                if (!mrow || mrow[j] != 0) att |= 1u << u;
            }
        }
    };
    // the first batch goes out before anything that waits for the previous kernel's results (q)
    load_prompt(0);
    {
        const T* q = static_cast<const T*>(a.q);
        const int per_head = G * hd;
        for (int idx = threadIdx.x; idx < 4 * per_head; idx += 256 * SH_WPH) {
            const int hq = idx / per_head, rem = idx - hq * per_head, g = rem / hd, d = rem - g * hd;
            const int head = blockIdx.y * 4 + hq;
            if (head < H) qs[hq][g][d] = (float)q[((int64_t)b * G + g) * a.ldq + head * hd + d];
        }
    }
    __syncthreads();

    float m[SH_GMAX], l[SH_GMAX], o[SH_GMAX][EPL];
#pragma unroll
    for (int g = 0; g < SH_GMAX; ++g) {
        m[g] = -FLT_MAX; l[g] = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[g][e] = 0.f;
    }
    // q . k of this lane's piece, summed over the LPK lanes of the key (every lane of the group ends up with the sum)
    auto dot = [&](const vec_t& kv, int g) -> float {
        float d = 0.f;
        if (active) {
            const float* qp = &qs[hh][g][EPL * dl];
#pragma unroll
            for (int e = 0; e < EPL; ++e) d = __builtin_fmaf(qp[e], (float)kv[e], d);
        }
#pragma unroll
        for (int off = LPK >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        return d * scale;
    };
    // fold one batch into row g's state: s[u] valid where bit u of `ok` is set
    auto update = [&](int g, const float (&s)[SH_U], unsigned ok) {
        float bm = -FLT_MAX;
#pragma unroll
        for (int u = 0; u < SH_U; ++u)
            if (ok >> u & 1) bm = fmaxf(bm, s[u]);
        bm = wave_max(bm);
        const float mn = fmaxf(m[g], bm), corr = __expf(m[g] - mn);
        m[g] = mn;
        l[g] *= corr;
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[g][e] *= corr;
#pragma unroll
        for (int u = 0; u < SH_U; ++u) {
            const float p = (ok >> u & 1) ? __expf(s[u] - mn) : 0.f;
            l[g] += p;
#pragma unroll
            for (int e = 0; e < EPL; ++e) o[g][e] = __builtin_fmaf(p, (float)vr[u][e], o[g][e]);
        }
    };

    // ---- prompt segment: every loaded key serves all G rows
    for (int j0 = 0; j0 < S0; j0 += STEP) {
        if (j0) load_prompt(j0);
#pragma unroll
        for (int g = 0; g < SH_GMAX; ++g) {
            if (g < G) {
                float s[SH_U];
#pragma unroll
                for (int u = 0; u < SH_U; ++u) s[u] = dot(kr[u], g);
                update(g, s, att);
            }
        }
    }

    // ---- tail segment: slot u = cc * G + g holds a key of row g; c = SH_U / G key groups per row and batch
    {
        const int n = t + 1, c = SH_U / G;
        T* kt = static_cast<T*>(a.kt);
        T* vt = static_cast<T*>(a.vt);
        const T* k_new = static_cast<const T*>(a.k_new);
        const T* v_new = static_cast<const T*>(a.v_new);
        for (int i0 = 0; i0 < n; i0 += c * SH_WPH * KPI) {
            float s[SH_U];
            unsigned ok = 0;
            int gu[SH_U];
#pragma unroll
            for (int u = 0; u < SH_U; ++u) {
                const int cc = u / G, g = u - cc * G;
                const int i = i0 + (cc * SH_WPH + part) * KPI + sub;
                gu[u] = g;
                kr[u] = (vec_t){}; vr[u] = (vec_t){};
                if (active && cc < c && i < n) {
                    const int64_t r = (int64_t)b * G + g;
                    const int64_t at = (r * a.t_max + i) * a.ldt + col;
                    if (i == t) {
                        kr[u] = *reinterpret_cast<const vec_t*>(k_new + r * a.ld_new + col);
                        vr[u] = *reinterpret_cast<const vec_t*>(v_new + r * a.ld_new + col);
                        *reinterpret_cast<vec_t*>(kt + at) = kr[u];
                        *reinterpret_cast<vec_t*>(vt + at) = vr[u];
                    } else {
                        kr[u] = *reinterpret_cast<const vec_t*>(kt + at);
                        vr[u] = *reinterpret_cast<const vec_t*>(vt + at);
                    }
                    ok |= 1u << u;
                }
            }
#pragma unroll
            for (int u = 0; u < SH_U; ++u) s[u] = dot(kr[u], gu[u]);
#pragma unroll
            for (int g = 0; g < SH_GMAX; ++g) {
                if (g < G) {
                    unsigned okg = 0;
#pragma unroll
                    for (int u = 0; u < SH_U; ++u)
                        if (gu[u] == g) okg |= ok & (1u << u);
                    update(g, s, okg);
                }
            }
        }
    }

    // ---- the keys of a wave are spread over its 64 / LPK sub-groups: sum them, then merge the waves of the head through LDS
#pragma unroll
    for (int g = 0; g < SH_GMAX; ++g) {
        if (g < G) {
#pragma unroll
            for (int off = LPK; off < 64; off <<= 1) {
                l[g] += __shfl_xor(l[g], off, 64);
#pragma unroll
                for (int e = 0; e < EPL; ++e) o[g][e] += __shfl_xor(o[g][e], off, 64);
            }
            if (sub == 0 && active) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) comb_o[hh][part][g][EPL * dl + e] = o[g][e];
            }
            if (lane == 0 && head_ok) { comb_m[hh][part][g] = m[g]; comb_l[hh][part][g] = l[g]; }
        }
    }
    __syncthreads();
    if (head_ok) {
        const int pieces = hd / EPL;
        T* out = static_cast<T*>(a.out);
        for (int item = part * 64 + lane; item < G * pieces; item += SH_WPH * 64) {
            const int g = item / pieces, pc = item - g * pieces;
            float mx = comb_m[hh][0][g];
#pragma unroll
            for (int w = 1; w < SH_WPH; ++w) mx = fmaxf(mx, comb_m[hh][w][g]);
            float den = 0.f, acc[EPL];
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
#pragma unroll
            for (int w = 0; w < SH_WPH; ++w) {
                const float wt = __expf(comb_m[hh][w][g] - mx);
                den = __builtin_fmaf(wt, comb_l[hh][w][g], den);
#pragma unroll
                for (int e = 0; e < EPL; ++e) acc[e] = __builtin_fmaf(wt, comb_o[hh][w][g][pc * EPL + e], acc[e]);
            }
            const float inv = 1.f / den;
            vec_t r;
#pragma unroll
            for (int e = 0; e < EPL; ++e) r[e] = (T)(acc[e] * inv);
            *reinterpret_cast<vec_t*>(out + ((int64_t)b * G + g) * a.ldo + h * hd + pc * EPL) = r;
        }
    }
}

// the status code of a call: what the kernel is told (filled by field name) plus the two arguments only the host reads
int validate(int dtype, int B, const SharedArgs& a) {
    if (!a.q || !a.kp || !a.vp || !a.kt || !a.vt || !a.k_new || !a.v_new || !a.out || B <= 0 || a.H <= 0) return EAVQA_E_ARG;
    if (dtype != EAVQA_BF16 && dtype != EAVQA_F32) return EAVQA_E_DTYPE;
    if (a.G < 1 || a.G > SH_GMAX || a.hd <= 0 || a.hd % 8 || a.hd > 128 || a.S0 < 1 || a.S0 > 3584 || a.t_max < 1 || a.t_max > 256 ||
        (a.H + 3) / 4 > 65535)
        return EAVQA_E_SHAPE;
    if (a.t < 0 || a.t >= a.t_max) return EAVQA_E_ARG;
    const int64_t unit = dtype == EAVQA_BF16 ? 8 : 4;          // elements in 16 bytes
    if (a.ldq % unit || a.ldk % unit || a.ldv % unit || a.ldt % unit || a.ld_new % unit || a.ldo % unit) return EAVQA_E_ALIGN;
    if (!eavqa_aligned16(a.q) || !eavqa_aligned16(a.kp) || !eavqa_aligned16(a.vp) || !eavqa_aligned16(a.kt) || !eavqa_aligned16(a.vt) ||
        !eavqa_aligned16(a.k_new) || !eavqa_aligned16(a.v_new) || !eavqa_aligned16(a.out))
        return EAVQA_E_ALIGN;
    const int64_t E = (int64_t)a.H * a.hd;
    if (a.ldq < E || a.ldk < E || a.ldv < E || a.ldt < E || a.ld_new < E || a.ldo < E || a.pbr < a.S0 || (a.key_mask && a.ld_mask < a.S0))
        return EAVQA_E_ARG;
    return EAVQA_OK;
}

}  // namespace

extern "C" int eavqa_attention_decode_shared(int dtype, int B, int G, int H, int S0, int t, int t_max, int hd, const void* q, int64_t ldq,
                                             const void* k_prompt, int64_t ldk, const void* v_prompt, int64_t ldv,
                                             int64_t prompt_batch_rows, void* k_tail, void* v_tail, int64_t ld_tail, const void* k_new,
                                             const void* v_new, int64_t ld_new, void* o, int64_t ldo, const int32_t* key_mask,
                                             int64_t ld_mask, float scale, void* stream) {
    SharedArgs a = {};
    a.q = q; a.ldq = ldq; a.kp = k_prompt; a.ldk = ldk; a.vp = v_prompt; a.ldv = ldv; a.pbr = prompt_batch_rows;
    a.kt = k_tail; a.vt = v_tail; a.ldt = ld_tail; a.k_new = k_new; a.v_new = v_new; a.ld_new = ld_new; a.out = o; a.ldo = ldo;
    a.key_mask = key_mask; a.ld_mask = ld_mask; a.G = G; a.H = H; a.S0 = S0; a.t = t; a.t_max = t_max; a.hd = hd; a.scale = scale;
    if (const int rc = validate(dtype, B, a)) return rc;
    // a lane takes 16 bytes of a key: LPK lanes cover hd <= 64 or hd <= 128 (static LDS only: nothing to opt into)
    const dim3 grid(B, (H + 3) / 4), block(256 * SH_WPH);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EAVQA_BF16) {
        if (hd <= 64) hipLaunchKernelGGL((attn_decode_shared_kernel<bf16_t, 8>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((attn_decode_shared_kernel<bf16_t, 16>), grid, block, 0, s, a);
    } else {
        if (hd <= 64) hipLaunchKernelGGL((attn_decode_shared_kernel<float, 16>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((attn_decode_shared_kernel<float, 32>), grid, block, 0, s, a);
    }
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
