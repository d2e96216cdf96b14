// Tracer of the decoder block drivers: runs csrc/lm_block.cpp and csrc/t5_block.cpp (compiled into this executable) against the recording
// stubs of stub.cpp on fixed cases and prints, per case, a header "== <case> rc=<return code> ws=<workspace bytes>" and then one line per
// kernel call.  Every pointer is a fake address the drivers never dereference; the workspace is exactly as large as the driver's own
// size function says.  tests/test_block_trace_cpu.py compares the output with tests/golden/block_trace.txt.
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "eavqa.h"
#include "eavqa_test.h"

extern std::string trace_log;
extern const char* trace_ws;

namespace {
template <class T = void> T* fake(uintptr_t a) { return reinterpret_cast<T*>(a); }
char* const WS = fake<char>(0x700000000000);          // above every other address of a case
void* const STREAM = fake(0x5000);
float* const X = fake<float>(0x10000000);
void* const OUT = fake(0x20000000);
const int32_t* const MASK = fake<int32_t>(0x30000000);
const float* const REL = fake<float>(0x40000000);
const float* const LN_FINAL = fake<float>(0x50000000);

// layer tables: structs of pointers only; field i of layer l gets the address (16 l + i + 1) MiB, so every table entry is distinct
template <class L, int N> struct Table {
    L layers[N];
    explicit Table(uintptr_t base) {
        void** p = reinterpret_cast<void**>(layers);
        const size_t fields = sizeof(L) / sizeof(void*);
        for (size_t i = 0; i < N * fields; ++i) p[i] = fake(base + (i / fields * 16 + i % fields + 1) * 0x100000);
    }
};
const Table<eavqa_lm_layer_t, 2> LM(0x100000000);
const Table<eavqa_lm_tail_t, 2> TAILS(0x200000000);
const Table<eavqa_t5_dec_layer_t, 2> T5(0x300000000);
const eavqa_lm_layer_scales_t SCALES[2] = {{0.5f, 0.25f, 0.125f, 2.f}, {1.5f, 0.75f, 0.375f, 3.f}};

void report(const char* name, int rc, int64_t ws) {
    printf("== %s rc=%d ws=%lld\n%s", name, rc, (long long)ws, trace_log.c_str());
    trace_log.clear();
}

const float EPS = 1e-5f;
const int ACT = EAVQA_ACT_RELU, S_MAX = 16, ROW0 = 5;

void lm(const char* name, int dtype, int n_layer, int E, int H, int F, int B, int Sq) {
    const int64_t ws = eavqa_lm_block_workspace_bytes(dtype, B * Sq, E, F);
    report(name, eavqa_lm_block_forward(dtype, n_layer, LM.layers, E, H, F, ACT, EPS, B, Sq, ROW0, S_MAX, X, MASK, S_MAX, WS, ws, STREAM), ws);
}
void lm_fp8(const char* name, int E, int H, int F, int B, int Sq) {
    const int64_t ws = eavqa_lm_block_fp8_workspace_bytes(B * Sq, E, F);
    report(name, eavqa_lm_block_forward_fp8(2, LM.layers, SCALES, E, H, F, ACT, EPS, B, Sq, ROW0, S_MAX, X, MASK, S_MAX, WS, ws, STREAM), ws);
}
void lm_shared(const char* name, int dtype, int B, int G) {
    const int E = 128, H = 4, F = 512;
    const int64_t ws = eavqa_lm_block_step_shared_workspace_bytes(dtype, B * G, E, F);
    report(name, eavqa_lm_block_step_shared(dtype, 2, LM.layers, TAILS.layers, E, H, F, ACT, EPS, B, G, ROW0, S_MAX, 2, 8, X, MASK, S_MAX, WS, ws,
                                            STREAM), ws);
}
// route < 0: eavqa_t5_decoder_step; otherwise eavqa_t5_decoder_step_ex with that route
void t5(const char* name, int dtype, int B, int inner, int H, int gated, const float* rel, int route) {
    const int E = 64, F = 128, t = 3, t_max = 8, S = 20;
    const int64_t ws = eavqa_t5_decoder_step_workspace_bytes(dtype, B, E, inner, F, gated);
    const int rc = route < 0 ? eavqa_t5_decoder_step(dtype, 2, T5.layers, LN_FINAL, E, inner, H, F, gated, EAVQA_ACT_GELU_NEW, 1e-6f, B, t, t_max, S, X,
                                                     OUT, MASK, S, rel, 2 * t_max - 1, t_max - 1, WS, ws, STREAM)
                             : eavqa_t5_decoder_step_ex(dtype, 2, T5.layers, LN_FINAL, E, inner, H, F, gated, EAVQA_ACT_GELU_NEW, 1e-6f, B, t, t_max, S,
                                                        X, OUT, MASK, S, rel, 2 * t_max - 1, t_max - 1, WS, ws, STREAM, route);
    report(name, rc, ws);
}
}

int main() {
    trace_ws = WS;
    const int BF = EAVQA_BF16, F32 = EAVQA_F32;
    lm("lm_bf16_decode", BF, 2, 128, 4, 512, 4, 1);
    lm("lm_bf16_decode_one_layer", BF, 1, 128, 4, 512, 4, 1);
    lm("lm_bf16_decode_hd144", BF, 2, 288, 2, 1152, 4, 1);
    lm("lm_bf16_prefill", BF, 2, 128, 4, 512, 4, 3);
    lm("lm_bf16_decode_B65", BF, 2, 128, 4, 512, 65, 1);
    lm("lm_f32_decode", F32, 2, 128, 4, 512, 4, 1);
    lm_fp8("lm_fp8_decode", 128, 4, 512, 4, 1);
    lm_fp8("lm_fp8_prefill", 128, 4, 512, 4, 3);
    lm_fp8("lm_fp8_decode_hd256", 256, 1, 1024, 4, 1);
    lm_shared("lm_shared_bf16_B2_G3", BF, 2, 3);
    lm_shared("lm_shared_bf16_B9_G8", BF, 9, 8);
    lm_shared("lm_shared_f32_B2_G2", F32, 2, 2);
    t5("t5_bf16_gated", BF, 4, 256, 4, 1, REL, -1);
    t5("t5_bf16_not_gated", BF, 4, 256, 4, 0, REL, -1);
    t5("t5_bf16_gated_route1", BF, 4, 256, 4, 1, REL, 1);
    t5("t5_bf16_not_gated_route1", BF, 4, 256, 4, 0, REL, 1);
    t5("t5_bf16_no_rel_bias", BF, 4, 256, 4, 1, nullptr, -1);
    t5("t5_f32", F32, 4, 256, 4, 1, REL, -1);
    t5("t5_bf16_B65", BF, 65, 256, 4, 1, REL, -1);
    t5("t5_bf16_inner224_H7", BF, 4, 224, 7, 1, REL, -1);
    {
        const int E = 64, inner = 256, H = 4, F = 128, B = 2, beams = 3, t = 3, t_max = 8, S = 20;
        const int64_t ws = eavqa_t5_decoder_step_beams_workspace_bytes(BF, B, beams, E, inner, F, 1);
        report("t5_beams_bf16_B2_beams3",
               eavqa_t5_decoder_step_beams(BF, 2, T5.layers, LN_FINAL, E, inner, H, F, 1, EAVQA_ACT_GELU_NEW, 1e-6f, B, beams, t, t_max, S, X, OUT, MASK,
                                           S, REL, 2 * t_max - 1, t_max - 1, WS, ws, STREAM), ws);
    }
    return 0;
}
