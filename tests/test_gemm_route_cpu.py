"""CPU: which kernel the GEMM dispatcher picks for a shape, pinned (csrc/gemm.hip route(), through the host-only eavqa_gemm_route of
include/eavqa_test.h).

ROUTES is a literal table (dtype, a_kc, b_kc, M, N, K, has_ln, knobs) -> (kind, index, split_rows): the shapes the dispatcher's own comments
and tools/gemm_shapes.py name, a pair of rows on either side of every threshold, every knob field at each documented value on a shape where
it changes the answer and on one where it must not, and eavqa_gemm_ln calls under the kernel selectors of tests/test_gemm_ln_gpu.py.  The
picks are the ones of the dispatcher as it was before it became a function (tools/gemm_route_trace.py replays the table on the GPU under a
kernel trace to tie the two together); a change here is a change of what a workload runs and needs a measurement.

What the table makes visible and nobody decided: an eavqa_gemm_ln call with the selector `big` (2 << 14), or one on a problem of four and
more rounds of 256 x 256 tiles, runs the general register-staged kernel - the round-1 kernels have no eavqa_gemm_ln form and the round-1
dispatch is where both end up."""
import ctypes as C

import pytest

F32, GEN, SKINNY, FAST, SHAPED, BIG, K64 = range(7)             # Kind, as include/eavqa_test.h numbers it
TABLE_SIZE = {F32: 4, GEN: 4, SKINNY: 1, FAST: 1, SHAPED: 5, BIG: 1, K64: 11}    # operand layouts, SHAPES, K64_SHAPES

ROUTES = [
    # shapes the dispatcher's comments name: M <= 64 at N = K = 2048, at K = 5120, at N = 10240
    ((1, 1, 1, 1, 2048, 2048, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 32, 2048, 2048, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 64, 2048, 2048, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 32, 2048, 5120, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 32, 10240, 2048, 0, 0), (K64, 5, 0)),
    ((1, 1, 1, 32, 6144, 2048, 0, 0), (K64, 5, 0)),
    # few-shot prefill (OPT-2.7B, M = 4 800): QKV, out-proj, FFN-up, FFN-down
    ((1, 1, 1, 4800, 7680, 2560, 0, 0), (K64, 4, 0)),
    ((1, 1, 1, 4800, 2560, 2560, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 4800, 10240, 2560, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 4800, 2560, 10240, 0, 0), (BIG, 0, 0)),
    # the CLIP tower (ViT-L/14) at 64 and at 160 images: QKV, out-proj, FFN-up, FFN-down
    ((1, 1, 1, 16448, 3072, 1024, 0, 0), (BIG, 0, 64)),
    ((1, 1, 1, 16448, 1024, 1024, 0, 0), (BIG, 0, 64)),
    ((1, 1, 1, 16448, 4096, 1024, 0, 0), (BIG, 0, 64)),
    ((1, 1, 1, 16448, 1024, 4096, 0, 0), (BIG, 0, 64)),
    ((1, 1, 1, 41120, 3072, 1024, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 41120, 1024, 1024, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 41120, 4096, 1024, 0, 0), (BIG, 0, 160)),
    ((1, 1, 1, 41120, 1024, 4096, 0, 0), (BIG, 0, 0)),
    # OPT-6.7B FFN-up at the few-shot prefill; 8192^3; the lm_head forward of GPT-2-large
    ((1, 1, 1, 4800, 16384, 4096, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 8192, 8192, 8192, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 1864, 50304, 1280, 0, 0), (BIG, 0, 72)),
    # the frozen LM's shapes of tools/gemm_shapes.py (GPT-2-large, packed M = 1 864)
    ((1, 1, 1, 1864, 1280, 5120, 0, 0), (K64, 5, 0)),
    ((1, 1, 1, 1864, 1280, 3840, 0, 0), (K64, 5, 0)),
    ((1, 1, 1, 1864, 3840, 1280, 0, 0), (K64, 3, 0)),
    ((1, 1, 1, 1864, 5120, 1280, 0, 0), (K64, 4, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0), (K64, 5, 0)),
    ((1, 1, 1, 1864, 1280, 50304, 0, 0), (K64, 5, 0)),
    # thresholds.  M 64 / 72
    ((1, 1, 1, 64, 2048, 2048, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 72, 2048, 2048, 0, 0), (K64, 5, 0)),
    # N 4096 / 4104 (few columns)
    ((1, 1, 1, 32, 4096, 2048, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 32, 4104, 2048, 0, 0), (K64, 5, 0)),
    # N 56 / 64
    ((1, 1, 1, 32, 56, 2080, 0, 0), (SHAPED, 0, 0)),
    ((1, 1, 1, 32, 64, 2080, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 32, 56, 2048, 0, 0), (K64, 5, 0)),
    ((1, 1, 1, 32, 64, 2048, 0, 0), (SKINNY, 0, 0)),
    # K % 64 == 0, K % 64 == 32, K % 32 != 0 (at M <= 64 and above)
    ((1, 1, 1, 300, 1280, 1280, 0, 0), (K64, 5, 0)),
    ((1, 1, 1, 300, 1280, 1312, 0, 0), (SHAPED, 0, 0)),
    ((1, 1, 1, 300, 1280, 1304, 0, 0), (GEN, 0, 0)),
    ((1, 1, 1, 32, 8192, 1280, 0, 0), (K64, 5, 0)),
    ((1, 1, 1, 32, 8192, 1312, 0, 0), (SKINNY, 0, 0)),
    ((1, 1, 1, 32, 8192, 1304, 0, 0), (GEN, 0, 0)),
    # 143 / 144 tiles of 256 x 256 (round-1 dispatch: k64_mode 1; without and with the shaped tiles, which win both)
    ((1, 1, 1, 2816, 3328, 1024, 0, 0x40100), (FAST, 0, 0)),
    ((1, 1, 1, 3072, 3072, 1024, 0, 0x40100), (BIG, 0, 0)),
    ((1, 1, 1, 2816, 3328, 1024, 0, 0x100), (SHAPED, 3, 0)),
    ((1, 1, 1, 3072, 3072, 1024, 0, 0x100), (SHAPED, 3, 0)),
    # 3 / 4 rounds of 256 x 256 tiles (both dispatchers pick the 256 x 256 kernel; an eavqa_gemm_ln call has only the general kernel left at 4)
    ((1, 1, 1, 6144, 8192, 1024, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 6400, 8192, 1024, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 6144, 8192, 1024, 1, 0), (BIG, 0, 0)),
    ((1, 1, 1, 6400, 8192, 1024, 1, 0), (GEN, 0, 0)),
    # 96 / 97 tile rows at 2 rounds
    ((1, 1, 1, 24576, 1024, 1024, 0, 0), (K64, 3, 0)),
    ((1, 1, 1, 24832, 1024, 1024, 0, 0), (BIG, 0, 0)),
    ((1, 1, 1, 24576, 1024, 1024, 1, 0), (K64, 3, 0)),
    ((1, 1, 1, 24832, 1024, 1024, 1, 0), (GEN, 0, 0)),
    # M % 256 = 192 / 200: the row split
    ((1, 1, 1, 16576, 1024, 1024, 0, 0), (BIG, 0, 192)),
    ((1, 1, 1, 16584, 1024, 1024, 0, 0), (K64, 4, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x100), (BIG, 0, 192)),
    ((1, 1, 1, 16584, 1024, 1024, 0, 0x100), (SHAPED, 3, 0)),
    # an operand that is not k-contiguous, bf16 and f32; f32 on a hot shape
    ((1, 0, 1, 304, 1280, 1280, 0, 0), (GEN, 2, 0)),
    ((1, 1, 0, 304, 1280, 1280, 0, 0), (GEN, 1, 0)),
    ((1, 0, 0, 304, 1280, 1280, 0, 0), (GEN, 3, 0)),
    ((1, 1, 0, 32, 2048, 2048, 0, 0), (GEN, 1, 0)),
    ((0, 1, 1, 304, 1280, 1280, 0, 0), (F32, 0, 0)),
    ((0, 0, 1, 304, 1280, 1280, 0, 0), (F32, 2, 0)),
    ((0, 1, 0, 304, 1280, 1280, 0, 0), (F32, 1, 0)),
    ((0, 0, 0, 304, 1280, 1280, 0, 0), (F32, 3, 0)),
    ((0, 1, 1, 32, 2048, 2048, 0, 0), (F32, 0, 0)),
    ((0, 1, 1, 16448, 4096, 1024, 0, 0), (F32, 0, 0)),
    # knobs.  stagger, ablate, deep, group_n: never the route
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x5), (K64, 5, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x5), (BIG, 0, 192)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x30), (K64, 5, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x30), (BIG, 0, 192)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x20000), (K64, 5, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x20000), (BIG, 0, 192)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x200000), (K64, 5, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x200000), (BIG, 0, 192)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x1200000), (K64, 5, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x1200000), (BIG, 0, 192)),
    # disable_fast: the general kernel (not for f32, which has no other)
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x80), (GEN, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x80), (GEN, 0, 0)),
    ((1, 1, 1, 32, 2048, 2048, 0, 0x80), (GEN, 0, 0)),
    ((0, 1, 1, 1864, 1280, 1280, 0, 0x80), (F32, 0, 0)),
    # k64_mode 1 (round-1 dispatch), 2.. (a forced tile, K % 64 == 0 only), beyond the table
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x100), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x100), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x200), (K64, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x200), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x300), (K64, 1, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x300), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x400), (K64, 2, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x400), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x500), (K64, 3, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x500), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x600), (K64, 4, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x600), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x700), (K64, 5, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x700), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x800), (K64, 6, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x800), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x900), (K64, 7, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x900), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0xa00), (K64, 8, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0xa00), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0xb00), (K64, 9, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0xb00), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0xc00), (K64, 10, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0xc00), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0xd00), (K64, 5, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0xd00), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x3f00), (K64, 5, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x3f00), (SHAPED, 0, 0)),
    ((1, 1, 1, 32, 8192, 1280, 0, 0x100), (SKINNY, 0, 0)),
    ((1, 1, 1, 32, 2048, 2048, 0, 0x700), (K64, 5, 0)),
    # big_mode 1 (never) / 2 (always, K % 64 == 0) / 3
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x4000), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x4000), (SHAPED, 0, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x4000), (SHAPED, 3, 0)),
    ((1, 1, 1, 41120, 4096, 1024, 0, 0x4000), (SHAPED, 2, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x8000), (BIG, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x8000), (SHAPED, 0, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x8000), (BIG, 0, 192)),
    ((1, 1, 1, 41120, 4096, 1024, 0, 0x8000), (BIG, 0, 160)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0xc000), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0xc000), (SHAPED, 0, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0xc000), (BIG, 0, 192)),
    ((1, 1, 1, 41120, 4096, 1024, 0, 0xc000), (BIG, 0, 160)),
    ((1, 1, 1, 32, 8192, 1280, 0, 0x8000), (BIG, 0, 0)),
    ((1, 1, 1, 32, 8192, 1280, 0, 0x8100), (SKINNY, 0, 0)),
    # shape_mode 1 (never) / 2..6 (always) / 7
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x40000), (FAST, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x40000), (FAST, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x80000), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x80000), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0xc0000), (SHAPED, 1, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0xc0000), (SHAPED, 1, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x100000), (SHAPED, 2, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x100000), (SHAPED, 2, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x140000), (SHAPED, 3, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x140000), (SHAPED, 3, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x180000), (SHAPED, 4, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x180000), (SHAPED, 4, 0)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x1c0000), (SHAPED, 0, 0)),
    ((1, 1, 1, 1864, 1280, 1312, 0, 0x1c0000), (SHAPED, 0, 0)),
    ((1, 1, 1, 32, 8192, 1312, 0, 0x80000), (SKINNY, 0, 0)),
    ((1, 1, 1, 300, 1280, 1304, 0, 0x80000), (GEN, 0, 0)),
    ((1, 1, 1, 1864, 1280, 5120, 0, 0x40100), (FAST, 0, 0)),
    ((1, 1, 1, 1864, 1280, 5120, 0, 0x100), (SHAPED, 0, 0)),
    # no_row_split
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x2000000), (K64, 4, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x2008000), (BIG, 0, 0)),
    ((1, 1, 1, 16576, 1024, 1024, 0, 0x8000), (BIG, 0, 192)),
    ((1, 1, 1, 1864, 1280, 1280, 0, 0x2000000), (K64, 5, 0)),
    # eavqa_gemm_ln calls x {auto, big, general, the K64 ids of tests/test_gemm_ln_gpu.py, a knob-only tile}: `big` reaches the general kernel
    ((1, 1, 1, 300, 1280, 256, 1, 0), (K64, 5, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0x8000), (GEN, 0, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0x80), (GEN, 0, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0x500), (K64, 3, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0x600), (K64, 4, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0x700), (K64, 5, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0xb00), (K64, 9, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0xc00), (K64, 10, 0)),
    ((1, 1, 1, 300, 1280, 256, 1, 0x200), (K64, 0, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0), (K64, 3, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0x8000), (GEN, 0, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0x80), (GEN, 0, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0x500), (K64, 3, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0x600), (K64, 4, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0x700), (K64, 5, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0xb00), (K64, 9, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0xc00), (K64, 10, 0)),
    ((1, 1, 1, 1943, 3840, 1280, 1, 0x200), (K64, 0, 0)),
    ((1, 1, 1, 32, 2048, 2048, 1, 0), (K64, 5, 0)),
    ((1, 1, 1, 70, 64, 64, 1, 0), (K64, 5, 0)),
    ((1, 1, 1, 16448, 4096, 1024, 1, 0), (GEN, 0, 0)),
    ((1, 1, 1, 41120, 4096, 1024, 1, 0), (GEN, 0, 0)),
    ((1, 1, 1, 300, 1280, 1312, 1, 0), (GEN, 0, 0)),
    ((0, 1, 1, 300, 1280, 256, 1, 0), (F32, 0, 0)),
]


@pytest.fixture(scope="module")
def route():
    from eavqa_amd import build, _lib
    build.build()
    lib = _lib.load()

    def f(dtype, a_kc, b_kc, M, N, K, has_ln, knobs):
        split = C.c_int(-1)
        r = lib.eavqa_gemm_route(dtype, a_kc, b_kc, M, N, K, has_ln, knobs, C.byref(split))
        return (r >> 8, r & 255, split.value) if r >= 0 else r
    return f


@pytest.mark.parametrize("row,want", ROUTES, ids=["-".join(f"{v:x}" if i == 7 else str(v) for i, v in enumerate(r)) + f"-{n}" for n, (r, _) in enumerate(ROUTES)])
def test_route_is_pinned(route, row, want):
    assert route(*row) == want


def test_shapes_no_kernel_takes_are_rejected_like_the_call(route):
    """eavqa_gemm_route answers with the code eavqa_gemm gives the shape (tests/test_abi.py pins those), and takes a null split_rows."""
    from eavqa_amd import _lib
    assert route(1, 1, 1, 8, 8, 132, 0, 0) == -3 and route(0, 1, 1, 8, 8, 130, 0, 0) == -3         # contiguous dimension % 8 (bf16) / % 4 (f32)
    assert route(1, 0, 1, 12, 8, 128, 0, 0) == -3 and route(1, 1, 0, 8, 12, 128, 0, 0) == -3
    assert route(1, 0, 1, 16, 8, 128, 1, 0) == -3                                                # eavqa_gemm_ln: k-contiguous operands only
    assert route(1, 1, 1, 0, 8, 128, 0, 0) == -1 and route(7, 1, 1, 8, 8, 128, 0, 0) == -4
    assert _lib.load().eavqa_gemm_route(1, 1, 1, 16576, 1024, 1024, 0, 0, None) == BIG * 256


def test_route_properties_on_random_shapes(route):
    """A few thousand pseudo-random shapes and knob words: a row split only on the 256 x 256 kernel and then exactly its ragged rows, the
    index inside its table, f32 on the f32 kernel whatever the knobs."""
    import random
    rng = random.Random(20240)
    seen = set()
    for _ in range(6000):
        dtype = rng.choice((1, 1, 1, 0))
        a_kc, b_kc = rng.choice(((1, 1), (1, 1), (1, 1), (1, 0), (0, 1), (0, 0)))
        M = rng.choice((rng.randint(1, 80), rng.randint(1, 3000), rng.randint(1, 50000))) * (1 if a_kc else 8)
        N = rng.choice((rng.randint(1, 700), rng.randint(1, 2000))) * 8
        K = rng.choice((rng.randint(1, 40) * 8, rng.randint(1, 160) * 32, rng.randint(1, 160) * 64))
        has_ln = int(a_kc and b_kc and rng.random() < 0.3)
        knobs = rng.choice((0, 0, rng.getrandbits(26), 1 << 8, 2 << 14, (1 << 8) | (1 << 18), 1 << 25))
        kind, index, split = route(dtype, a_kc, b_kc, M, N, K, has_ln, knobs)
        seen.add(kind)
        assert 0 <= index < TABLE_SIZE[kind]
        if kind == BIG:
            assert split == 0 or (0 < split <= 192 and split == M % 256)
        else:
            assert split == 0
        if dtype == 0:
            assert kind == F32
        if kind in (F32, GEN):
            assert index == 2 * (not a_kc) + (not b_kc)
    assert seen == set(range(7))
