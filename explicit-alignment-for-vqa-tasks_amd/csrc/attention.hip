// Attention host layer (eavqa_attention_* in include/eavqa.h and include/eavqa_test.h): argument validation, the two dispatchers that
// choose a kernel, and the entry points, which only describe their call (AttnCall, attention_params.h).  The kernels and their launch
// code are included below, into this one translation unit.
#include "attention_params.h"
#include "attention_valu.hip"     // fp32 arithmetic on the vector ALU, both storage types: the parity path
#include "attention_decode.hip"   // bf16, one query per sample against a K / V cache
#include "attention_mfma.hip"     // bf16 matrix-core kernels

namespace {

namespace mfma = eavqa_attn_mfma;

// Everything the entry points have in common, in the order their callers rely on (tests/test_abi.py pins the codes); fills in the
// defaults of ld_mask / bsq / bsk and the pitch of the statistics.  Leading dimensions a pass does not use are 0.
int validate(AttnCall& c, bool backward) {
    AttnParams& p = c.p;
    if ((!p.q && !c.qkv_part) || !p.k || !p.v) return EAVQA_E_ARG;
    if (backward ? (!p.o || !p.d_o || !p.dq || !p.dk || !p.dv || !p.lse || !p.delta) : !p.out) return EAVQA_E_ARG;
    if (p.B <= 0 || p.H <= 0 || p.Sq <= 0 || p.Sk <= 0 || p.hd <= 0) return EAVQA_E_ARG;
    if (c.dtype != EAVQA_F32 && c.dtype != EAVQA_BF16) return EAVQA_E_DTYPE;
    if (p.hd % 4 || (int64_t)p.B * p.H > 65535) return EAVQA_E_SHAPE;
    if (p.ldq % 4 || p.ldk % 4 || p.ldv % 4 || p.ldo % 4 || p.lddo % 4 || p.lddq % 4 || p.lddk % 4 || p.lddv % 4) return EAVQA_E_ALIGN;
    // eavqa_attention_fwd_rel / _bwd_rel: the table must span -(Sk - 1) .. Sk - 1
    if (c.rel_route && p.rel_bias && (p.rel_zero < p.Sk - 1 || p.rel_ld < p.rel_zero + p.Sk)) return EAVQA_E_ARG;
    if (p.cu && (p.key_mask || p.Sq != p.Sk)) return EAVQA_E_ARG;
    if (p.ld_mask <= 0) p.ld_mask = p.Sk;
    if (p.ld_mask < p.Sk) return EAVQA_E_ARG;
    if (p.bsq <= 0) p.bsq = p.Sq;
    if (p.bsk <= 0) p.bsk = p.Sk;
    if (p.bsq < p.Sq || p.bsk < p.Sk) return EAVQA_E_ARG;
    p.stat_ld = p.Sq;
    return EAVQA_OK;
}

bool mult8(std::initializer_list<int64_t> lds) { for (int64_t ld : lds) if (ld % 8) return false; return true; }
bool aligned16(std::initializer_list<const void*> ptrs) { for (const void* ptr : ptrs) if (!eavqa_aligned16(ptr)) return false; return true; }

int run_valu(Pass pass, AttnCall& c) {            // launch_cfg sets c.p.tile
    return c.dtype == EAVQA_F32 ? dispatch<float>(pass, c.p, c.stream) : dispatch<bf16_t>(pass, c.p, c.stream);
}

// Routing.  This table is the specification: the dispatchers below implement it and nothing else.  Path bits: include/eavqa_test.h
// (bit 0 = the VALU bit); "supported" = mfma::supported(hd): hd 64 / 80 / 96 / 128; "wide" = mfma::supported_wide: hd > 128, a
// multiple of 8, Sq and Sk <= 64.
//
// Forward, plain route (eavqa_attention_fwd / _fwd_ex / _decode / _decode_splitk / _decode_splitk_rel; _fwd_rel without a bias, which
//                       comes with path 0 and no cu):
//   1. decode kernel      decode_supported, VALU bit clear, q (or the partial sums), k, v and o 16-byte aligned
//      otherwise          the append and partial-sum forms: EAVQA_E_SHAPE; a bias: EAVQA_E_SHAPE
//   2. bf16, VALU bit clear, in this order
//        wide one-tile    wide, ldq / ldk / ldv multiples of 8
//        K/V-resident     supported, path bit 2 clear, Sk > 64 or path bit 3, resident_supported
//        streamed MFMA    supported
//   3. VALU kernels
// Forward, rel route (eavqa_attention_fwd_rel with a bias):
//   1. streamed MFMA      bf16, supported, ldq / ldk / ldv multiples of 8, q / k / v 16-byte aligned (never resident or wide)
//   2. VALU kernels
//
// Backward, plain route (eavqa_attention_bwd / _bwd_ex):
//   1. bf16, VALU bit clear, in this order (no pointer-alignment condition)
//        wide one-tile    wide, ldq / ldk / ldv / ldo / lddo multiples of 8
//        fused one-tile   supported, Sq and Sk <= 64, path bit 1 (split) clear; fused_padded = path bit 2
//        dQ, then dK/dV   supported
//   2. VALU kernels: dQ, then dK/dV
// Backward, rel route (eavqa_attention_bwd_rel, with or without a bias; no path bits, no wide kernel):
//   1. bf16, supported, all eight leading dimensions multiples of 8, all eight tensors 16-byte aligned:
//        fused one-tile   Sq and Sk <= 64
//        dQ, then dK/dV
//   2. VALU kernels: dQ, then dK/dV
int attention_forward(const AttnCall& call) {
    AttnCall c = call;
    if (int rc = validate(c, false)) return rc;
    AttnParams& p = c.p;
    const bool bf16 = c.dtype == EAVQA_BF16, valu_bit = (c.path & 1) != 0;
    if (c.rel_route) {
        if (bf16 && mfma::supported(p.hd) && mult8({p.ldq, p.ldk, p.ldv}) && aligned16({p.q, p.k, p.v})) return mfma::run(Pass::Fwd, p, c.stream);
        return run_valu(Pass::Fwd, c);
    }
    if (decode_supported(c) && !valu_bit && (c.qkv_part || eavqa_aligned16(p.q)) && aligned16({p.k, p.v, p.out})) return launch_decode(c);
    if (c.k_new || c.v_new || c.qkv_part) return EAVQA_E_SHAPE;     // the append forms exist for the decode kernel only
    if (p.rel_bias) return EAVQA_E_SHAPE;                           // (a bias reaches the tiled kernels on the rel route only)
    if (bf16 && !valu_bit) {
        if (mfma::supported_wide(p.hd, p.Sq, p.Sk) && mult8({p.ldq, p.ldk, p.ldv})) return mfma::run_wide(Pass::Fwd, p, c.stream);
        if (mfma::supported(p.hd)) {
            // K / V resident in LDS (the CLIP tower: one workgroup per (image, head)); path bit 2 keeps the streamed-tile kernel (A / B, tests)
            if (!(c.path & 4) && (p.Sk > 64 || (c.path & 8)) && mfma::resident_supported(p)) return mfma::run_resident(p, c.stream);
            return mfma::run(Pass::Fwd, p, c.stream);
        }
    }
    return run_valu(Pass::Fwd, c);
}

int attention_backward(const AttnCall& call) {
    AttnCall c = call;
    if (int rc = validate(c, true)) return rc;
    AttnParams& p = c.p;
    const bool bf16 = c.dtype == EAVQA_BF16;
    bool wide = false, on_mfma, fused = p.Sq <= mfma::TILE && p.Sk <= mfma::TILE;
    if (c.rel_route) {
        on_mfma = bf16 && mfma::supported(p.hd) && mult8({p.ldq, p.ldk, p.ldv, p.ldo, p.lddo, p.lddq, p.lddk, p.lddv}) &&
                  aligned16({p.q, p.k, p.v, p.o, p.d_o, p.dq, p.dk, p.dv});
    } else {
        wide = mfma::supported_wide(p.hd, p.Sq, p.Sk) && mult8({p.ldq, p.ldk, p.ldv, p.ldo, p.lddo});
        on_mfma = bf16 && (mfma::supported(p.hd) || wide) && !(c.path & 1);
        fused = fused && !(c.path & 2);                 // path bit 1: two-kernel backward even when the problem is one tile
        p.fused_padded = (c.path & 4) != 0;             // path bit 2: the round-2 padded-pitch one-tile kernel also for hd = 64
    }
    if (on_mfma) {
        if (wide) return mfma::run_wide(Pass::BwdFused, p, c.stream);
        if (fused) return mfma::run(Pass::BwdFused, p, c.stream);
        if (int rc = mfma::run(Pass::BwdDq, p, c.stream)) return rc;
        return mfma::run(Pass::BwdDkv, p, c.stream);
    }
    if (int rc = run_valu(Pass::BwdDq, c)) return rc;
    return run_valu(Pass::BwdDkv, c);
}

}  // namespace

extern "C" int eavqa_attention_fwd_ex(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                      const void* v, int64_t ldv, void* o, int64_t ldo, int64_t q_batch_rows, int64_t kv_batch_rows,
                                      const int32_t* key_mask, int64_t ld_mask, const int32_t* cu_seqlens, int causal, float scale,
                                      float* lse, void* stream, int path) {
    AttnCall c = {};
    c.dtype = dtype; c.stream = reinterpret_cast<hipStream_t>(stream); c.path = path;
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = Sq; p.Sk = Sk; p.hd = hd; p.causal = causal; p.scale = scale;
    p.q = q; p.ldq = ldq; p.k = k; p.ldk = ldk; p.v = v; p.ldv = ldv; p.out = o; p.ldo = ldo; p.lse = lse;
    p.bsq = q_batch_rows; p.bsk = kv_batch_rows; p.key_mask = key_mask; p.ld_mask = ld_mask; p.cu = cu_seqlens;
    return attention_forward(c);
}

extern "C" int eavqa_attention_fwd(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                   const void* v, int64_t ldv, void* o, int64_t ldo, int64_t q_batch_rows, int64_t kv_batch_rows,
                                   const int32_t* key_mask, int64_t ld_mask, const int32_t* cu_seqlens, int causal, float scale,
                                   float* lse, void* stream) {
    return eavqa_attention_fwd_ex(dtype, B, H, Sq, Sk, hd, q, ldq, k, ldk, v, ldv, o, ldo, q_batch_rows, kv_batch_rows, key_mask,
                                  ld_mask, cu_seqlens, causal, scale, lse, stream, 0);
}

// The three decode forms are a causal forward of one query per sample (Sq = q_batch_rows = 1) that only the decode kernel can serve.
extern "C" int eavqa_attention_decode(int dtype, int B, int H, int Sk, int hd, const void* q, int64_t ldq, void* k_cache, int64_t ldk,
                                      void* v_cache, int64_t ldv, int64_t kv_batch_rows, const void* k_new, const void* v_new,
                                      int64_t ld_new, void* o, int64_t ldo, const int32_t* key_mask, int64_t ld_mask, float scale,
                                      void* stream) {
    if (!k_new || !v_new) return EAVQA_E_ARG;
    if (ld_new % 8 || !eavqa_aligned16(k_new) || !eavqa_aligned16(v_new)) return EAVQA_E_ALIGN;
    AttnCall c = {};
    c.dtype = dtype; c.stream = reinterpret_cast<hipStream_t>(stream);
    c.k_new = k_new; c.v_new = v_new; c.ld_new = ld_new;
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = 1; p.Sk = Sk; p.hd = hd; p.causal = 1; p.scale = scale;
    p.q = q; p.ldq = ldq; p.k = k_cache; p.ldk = ldk; p.v = v_cache; p.ldv = ldv; p.out = o; p.ldo = ldo;
    p.bsq = 1; p.bsk = kv_batch_rows; p.key_mask = key_mask; p.ld_mask = ld_mask;
    return attention_forward(c);
}

extern "C" int eavqa_attention_decode_splitk(int dtype, int B, int H, int Sk, int hd, const float* qkv_partials, int ks, const float* qkv_bias,
                                             void* k_cache, int64_t ldk, void* v_cache, int64_t ldv, int64_t kv_batch_rows, void* o, int64_t ldo,
                                             const int32_t* key_mask, int64_t ld_mask, float scale, void* stream) {
    if (!qkv_partials || ks <= 0) return EAVQA_E_ARG;
    if ((H * hd) % 4 || !eavqa_aligned16(qkv_partials) || (qkv_bias && !eavqa_aligned16(qkv_bias))) return EAVQA_E_ALIGN;
    AttnCall c = {};
    c.dtype = dtype; c.stream = reinterpret_cast<hipStream_t>(stream);
    c.qkv_part = qkv_partials; c.ks = ks; c.qkv_bias = qkv_bias;
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = 1; p.Sk = Sk; p.hd = hd; p.causal = 1; p.scale = scale;
    p.ldq = 8;                                    // q does not exist yet: it is summed up from the partial sums
    p.k = k_cache; p.ldk = ldk; p.v = v_cache; p.ldv = ldv; p.out = o; p.ldo = ldo;
    p.bsq = 1; p.bsk = kv_batch_rows; p.key_mask = key_mask; p.ld_mask = ld_mask;
    return attention_forward(c);
}

extern "C" int eavqa_attention_decode_splitk_rel(int dtype, int B, int H, int Sk, int hd, const float* partials, int ks, int part_cols,
                                                 void* k, int64_t ldk, void* v, int64_t ldv, int64_t kv_batch_rows, void* o, int64_t ldo,
                                                 const int32_t* key_mask, int64_t ld_mask, float scale, const float* rel_bias, int64_t rel_ld,
                                                 int rel_zero, void* stream) {
    if (!partials || ks <= 0) return EAVQA_E_ARG;
    if (part_cols != H * hd && part_cols != 3 * H * hd) return EAVQA_E_SHAPE;
    if ((H * hd) % 4 || !eavqa_aligned16(partials)) return EAVQA_E_ALIGN;
    if (rel_bias && (rel_zero < Sk - 1 || rel_ld < rel_zero + 1)) return EAVQA_E_ARG;     // offsets -(Sk - 1) .. 0 are read
    AttnCall c = {};
    c.dtype = dtype; c.stream = reinterpret_cast<hipStream_t>(stream);
    c.qkv_part = partials; c.ks = ks; c.part_cols = part_cols;
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = 1; p.Sk = Sk; p.hd = hd; p.causal = 1; p.scale = scale;
    p.ldq = 8;                                    // as in eavqa_attention_decode_splitk
    p.k = k; p.ldk = ldk; p.v = v; p.ldv = ldv; p.out = o; p.ldo = ldo;
    p.bsq = 1; p.bsk = kv_batch_rows; p.key_mask = key_mask; p.ld_mask = ld_mask;
    p.rel_bias = rel_bias; p.rel_ld = rel_ld; p.rel_zero = rel_zero;
    return attention_forward(c);
}

// The decode kernel's plan of a shape, for the tests (include/eavqa_test.h): validate() on a bf16 call of one query per sample whose
// pointers and leading dimensions are in order, the kernel's domain (outside it the decode forms are EAVQA_E_SHAPE), then decode_plan().
// variant = (lanes per key, waves per head, loads in flight, V mode).
extern "C" int eavqa_attention_decode_route(int B, int H, int Sk, int hd, int path, eavqa_launch_plan_t* out) {
    AttnCall c = {};
    c.dtype = EAVQA_BF16; c.path = path;
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = 1; p.Sk = Sk; p.hd = hd; p.causal = 1; p.bsq = 1;
    p.q = p.k = p.v = p.out = reinterpret_cast<void*>(uintptr_t(16));     // (aligned, never dereferenced)
    p.ldq = p.ldk = p.ldv = p.ldo = (int64_t)H * hd;
    if (const int rc = validate(c, false)) return rc;
    if (!decode_supported(c) || (path & 1)) return EAVQA_E_SHAPE;
    const DecodePlan d = decode_plan(c);
    report(out, d.lpk, d.wph, d.u, d.vmode, d.grid, d.block, d.lds);
    return EAVQA_OK;
}

#ifdef EAVQA_ATTN_STAMPS
extern "C" __attribute__((visibility("default"))) int eavqa_attn_stamps_read(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(eavqa_attn_stamps), sizeof(unsigned long long) * 256) == hipSuccess ? 0 : -5;
}
#endif

extern "C" int eavqa_attention_bwd_ex(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                      const void* v, int64_t ldv, const void* o, int64_t ldo, const void* d_o, int64_t lddo,
                                      void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                                      const int32_t* key_mask, const int32_t* cu_seqlens, int causal, float scale,
                                      const float* lse, float* delta, void* stream, int path) {
    AttnCall c = {};
    c.dtype = dtype; c.stream = reinterpret_cast<hipStream_t>(stream); c.path = path;
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = Sq; p.Sk = Sk; p.hd = hd; p.causal = causal; p.scale = scale;
    p.q = q; p.ldq = ldq; p.k = k; p.ldk = ldk; p.v = v; p.ldv = ldv; p.o = o; p.ldo = ldo; p.d_o = d_o; p.lddo = lddo;
    p.dq = dq; p.lddq = lddq; p.dk = dk; p.lddk = lddk; p.dv = dv; p.lddv = lddv;
    p.key_mask = key_mask; p.cu = cu_seqlens; p.lse = const_cast<float*>(lse); p.delta = delta;
    return attention_backward(c);
}

extern "C" int eavqa_attention_bwd(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                   const void* v, int64_t ldv, const void* o, int64_t ldo, const void* d_o, int64_t lddo,
                                   void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                                   const int32_t* key_mask, const int32_t* cu_seqlens, int causal, float scale,
                                   const float* lse, float* delta, void* stream) {
    return eavqa_attention_bwd_ex(dtype, B, H, Sq, Sk, hd, q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, dq, lddq, dk, lddk, dv, lddv,
                                  key_mask, cu_seqlens, causal, scale, lse, delta, stream, 0);
}

// ---------------------------------------------------------------------------------------------------- T5 relative-position bias
// eavqa_attention_fwd / _bwd with an additive per-head bias that depends on (key position - query position) only: T5's relative
// attention bias (HF:models/t5/modeling_t5.py:217-279 - compute_bias: values[h][q][k] = table[bucket(k - q)][h], shared by every layer
// of a stack) handed over as rel_bias[h * rel_ld + (k - q) + rel_zero], float32, q counted from the END of the keys when Sq < Sk (a
// cached decode step: query i sits at position i + Sk - Sq).  bf16 at an MFMA head size takes the matrix-core kernels, which add the
// bias to their score tiles (T0_3B few-shot: the vector-ALU forward was 27 % of the GPU time, 71 us per call; its backward 12 % of a
// training step); everything else is fp32 arithmetic on the vector-ALU kernels.
extern "C" int eavqa_attention_fwd_rel(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                       const void* v, int64_t ldv, void* o, int64_t ldo, int64_t q_batch_rows, int64_t kv_batch_rows,
                                       const int32_t* key_mask, int64_t ld_mask, int causal, float scale, const float* rel_bias,
                                       int64_t rel_ld, int rel_zero, float* lse, void* stream) {
    AttnCall c = {};
    c.dtype = dtype; c.stream = reinterpret_cast<hipStream_t>(stream);
    c.rel_route = rel_bias != nullptr;            // without a bias this is eavqa_attention_fwd (T5's cross-attention)
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = Sq; p.Sk = Sk; p.hd = hd; p.causal = causal; p.scale = scale;
    p.q = q; p.ldq = ldq; p.k = k; p.ldk = ldk; p.v = v; p.ldv = ldv; p.out = o; p.ldo = ldo; p.lse = lse;
    p.bsq = q_batch_rows; p.bsk = kv_batch_rows; p.key_mask = key_mask; p.ld_mask = ld_mask;
    p.rel_bias = rel_bias; p.rel_ld = rel_ld; p.rel_zero = rel_zero;
    return attention_forward(c);
}

extern "C" int eavqa_attention_bwd_rel(int dtype, int B, int H, int Sq, int Sk, int hd, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                       const void* v, int64_t ldv, const void* o, int64_t ldo, const void* d_o, int64_t lddo,
                                       void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                                       const int32_t* key_mask, int causal, float scale, const float* rel_bias, int64_t rel_ld,
                                       int rel_zero, const float* lse, float* delta, void* stream) {
    AttnCall c = {};
    c.dtype = dtype; c.stream = reinterpret_cast<hipStream_t>(stream);
    c.rel_route = true;                           // also without a bias
    AttnParams& p = c.p;
    p.B = B; p.H = H; p.Sq = Sq; p.Sk = Sk; p.hd = hd; p.causal = causal; p.scale = scale;
    p.q = q; p.ldq = ldq; p.k = k; p.ldk = ldk; p.v = v; p.ldv = ldv; p.o = o; p.ldo = ldo; p.d_o = d_o; p.lddo = lddo;
    p.dq = dq; p.lddq = lddq; p.dk = dk; p.lddk = lddk; p.dv = dv; p.lddv = lddv;
    p.key_mask = key_mask; p.lse = const_cast<float*>(lse); p.delta = delta;
    p.rel_bias = rel_bias; p.rel_ld = rel_ld; p.rel_zero = rel_zero;
    return attention_backward(c);
}
