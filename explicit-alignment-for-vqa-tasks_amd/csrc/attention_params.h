// What every attention kernel is told about its problem, shared by attention_valu.hip, attention_mfma.hip and the host layer in
// attention.hip (one translation unit).
#pragma once
#include "common.h"

namespace {            // this header is private to attention.hip's translation unit

struct AttnParams {
    const void* q; const void* k; const void* v; const void* o; const void* d_o;
    void* out;   // fwd: o
    void* dq; void* dk; void* dv;
    int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    const int32_t* key_mask; int64_t ld_mask;
    const int32_t* cu;   // packed self-attention: sample b owns rows [cu[b], cu[b+1]) of q/k/v/o (Sq = Sk = that length)
    float* lse; float* delta;
    int B, H, Sq, Sk, hd, causal;
    int stat_ld;         // row pitch of lse / delta: [B, H, stat_ld]
    int fused_padded;    // one-tile MFMA backward, hd 64: keep the round-2 padded-pitch kernel (eavqa_attention_bwd_ex path bit 2: A / B, parity)
    int64_t bsq, bsk;   // rows between consecutive batches of q/o/do/dq and of k/v/dk/dv
    int tile;            // vector-ALU kernels: rows per LDS tile (set by launch_cfg)
    float scale;
    // T5 relative-position bias (eavqa_attention_fwd_rel / _bwd_rel): score(i, j) += rel_bias[h * rel_ld + (j - (i + Sk - Sq)) + rel_zero]
    const float* rel_bias; int64_t rel_ld; int rel_zero;
};

// T5's additive relative-position bias of (head h, key position, query position counted from the end of the keys): 0 without a table;
// entries outside the table are clamped (they belong to masked positions, or to rows / keys beyond the sequence, only).  Used by the
// forward AND, since round 4, by the backward kernels (the frozen T5's dgrad recomputes P = softmax(q k^T scale + bias): T0_3B training
// spent 12 % of its step in the vector-ALU backward kernels because only they knew the bias).
__device__ __forceinline__ float rel_bias_at(const AttnParams& p, int h, int key, int qpos) {
    if (!p.rel_bias) return 0.f;
    const int idx = min(max(key - qpos + p.rel_zero, 0), (int)p.rel_ld - 1);
    return p.rel_bias[(int64_t)h * p.rel_ld + idx];
}

// which kernel of a family: forward, dQ (+ delta), dK / dV, or all three gradients of a one-tile problem (Sq, Sk <= 64)
enum class Pass { Fwd, BwdDq, BwdDkv, BwdFused };

// One call of an attention entry point, as the host layer sees it (attention.hip: attention_forward / attention_backward).  Zero-
// initialise it and name what you set.  p.ld_mask, p.bsq and p.bsk may stay 0 (= Sk, Sq, Sk); p.stat_ld and p.tile are filled in on the way.
struct AttnCall {
    AttnParams p;
    int dtype;
    hipStream_t stream;
    int path;            // kernel-selection bits of include/eavqa_test.h (0 from the public entry points)
    // The _rel entry points' own route: only the tiled MFMA kernels (no decode, wide or K/V-resident kernel), and only when every
    // leading dimension is a multiple of 8 and every pointer 16-byte aligned; no path bits.  eavqa_attention_fwd_rel sets it when it has a
    // bias (without one it is eavqa_attention_fwd), eavqa_attention_bwd_rel always.
    bool rel_route;
    // decode kernel only (attention_decode.hip): the new position's K / V rows to append, or the QKV projection's split-K partial sums
    const void* k_new; const void* v_new; int64_t ld_new;
    const float* qkv_part; int ks; const float* qkv_bias; int part_cols;
};

}  // namespace
