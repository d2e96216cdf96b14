"""CPU: which kernel variant, grid, workgroup and LDS size the decode-step kernels get for a shape, pinned (the plan functions of
csrc/decode_params.h, through the host-only eavqa_gemm_splitk_route / eavqa_gemm_decode_route / eavqa_attention_decode_route of
include/eavqa_test.h).

Three literal tables, row -> (variant, (grid x, grid y), workgroup, LDS bytes) or the EAVQA_E_* code the shape and selector earn: the
shapes the flagship workloads run (OPT-2.7B and T0-3B decode steps at 32 rows), a pair of rows on either side of every threshold, every
selector field at each legal value and at one illegal one.  The picks were read off the launchers as they stood before the choice became a
function of its own; a change here is a change of what a workload runs and needs a measurement.  The selector of the e4m3 split-K kernel
exists in the route alone (its entry point has none): its legal values are the instantiated kernels."""
import ctypes as C

import pytest

ARG, SHAPE, DTYPE = -1, -3, -4

# (fp8, M, N, K, ks, sel) -> ((16-row fragments, fragments per wave, waves, k-steps in flight), grid, workgroup, LDS bytes)
SPLITK = [
    # OPT-2.7B at M = 32, the planned ks: QKV, out-proj, FFN-up, FFN-down; bf16, then e4m3
    ((0, 32, 7680, 2560, 4, 0), ((2, 1, 8, 16), (60, 4), 512, 40960)),
    ((0, 32, 2560, 2560, 10, 0), ((2, 1, 8, 8), (20, 10), 512, 16384)),
    ((0, 32, 10240, 2560, 5, 0), ((2, 1, 8, 16), (80, 5), 512, 32768)),
    ((0, 32, 2560, 10240, 10, 0), ((2, 1, 8, 16), (20, 10), 512, 65536)),
    ((1, 32, 7680, 2560, 4, 0), ((2, 1, 8, 4), (60, 4), 512, 20480)),
    ((1, 32, 2560, 2560, 5, 0), ((2, 1, 8, 4), (20, 5), 512, 16384)),
    ((1, 32, 10240, 2560, 2, 0), ((2, 1, 8, 8), (80, 2), 512, 40960)),
    ((1, 32, 2560, 10240, 10, 0), ((2, 1, 8, 8), (20, 10), 512, 32768)),
    # a T0-3B decoder step at 32 rows (E = inner = 2048, F = 5120, gated): QKV, out-proj / cross-attention q, [wi_0; wi_1], wo
    ((0, 32, 6144, 2048, 4, 0), ((2, 1, 8, 16), (48, 4), 512, 32768)),
    ((0, 32, 2048, 2048, 8, 0), ((2, 1, 8, 8), (16, 8), 512, 16384)),
    ((0, 32, 10240, 2048, 2, 0), ((2, 1, 8, 16), (80, 2), 512, 65536)),
    ((0, 32, 2048, 5120, 16, 0), ((2, 1, 8, 8), (16, 16), 512, 20480)),
    # M 1, 16 / 17, 32 / 33, 64
    ((0, 1, 2560, 2560, 10, 0), ((1, 1, 8, 8), (20, 10), 512, 8192)),
    ((0, 16, 2560, 2560, 10, 0), ((1, 1, 8, 8), (20, 10), 512, 8192)),
    ((0, 17, 2560, 2560, 10, 0), ((2, 1, 8, 8), (20, 10), 512, 16384)),
    ((0, 33, 2560, 2560, 10, 0), ((4, 1, 8, 8), (20, 10), 512, 32768)),
    ((0, 64, 2560, 2560, 10, 0), ((4, 1, 8, 8), (20, 10), 512, 32768)),
    ((1, 1, 2560, 2560, 5, 0), ((1, 1, 8, 4), (20, 5), 512, 8192)),
    ((1, 16, 2560, 2560, 5, 0), ((1, 1, 8, 4), (20, 5), 512, 8192)),
    ((1, 17, 2560, 2560, 5, 0), ((2, 1, 8, 4), (20, 5), 512, 16384)),
    ((1, 33, 2560, 2560, 5, 0), ((4, 1, 8, 4), (20, 5), 512, 32768)),
    ((1, 64, 2560, 2560, 5, 0), ((4, 1, 8, 4), (20, 5), 512, 32768)),
    # the deep window: slices of 512 / 480 values (bf16), 1024 / 896 (e4m3)
    ((0, 32, 2560, 2048, 4, 0), ((2, 1, 8, 16), (20, 4), 512, 32768)),
    ((0, 32, 2560, 1920, 4, 0), ((2, 1, 8, 8), (20, 4), 512, 30720)),
    ((1, 32, 2560, 4096, 4, 0), ((2, 1, 8, 8), (20, 4), 512, 32768)),
    ((1, 32, 2560, 3584, 4, 0), ((2, 1, 8, 4), (20, 4), 512, 28672)),
    # selector (eavqa_gemm_splitk_ex `unroll`): k-steps 8 / 16, waves 4 / 8, fragments 1 / 2, two fields at once, bits above the fields
    ((0, 32, 2560, 2560, 10, 8), ((2, 1, 8, 8), (20, 10), 512, 16384)),
    ((0, 32, 2560, 2560, 10, 16), ((2, 1, 8, 16), (20, 10), 512, 16384)),
    ((0, 32, 2560, 2560, 10, 0x400), ((2, 1, 4, 8), (40, 10), 256, 16384)),
    ((0, 32, 2560, 2560, 10, 0x800), ((2, 1, 8, 8), (20, 10), 512, 16384)),
    ((0, 32, 2560, 2560, 10, 0x1000), ((2, 1, 8, 8), (20, 10), 512, 16384)),
    ((0, 32, 2560, 2560, 10, 0x2000), ((2, 2, 8, 8), (10, 10), 512, 16384)),
    ((0, 32, 2560, 2560, 10, 0x2410), ((2, 2, 4, 16), (20, 10), 256, 16384)),
    ((0, 32, 2560, 2560, 10, 0x10010), ((2, 1, 8, 16), (20, 10), 512, 16384)),
    ((0, 32, 2560, 2560, 10, 4), ARG),
    ((0, 32, 2560, 2560, 10, 0x200), ARG),
    ((0, 32, 2560, 2560, 10, 0x3000), ARG),
    # ... of the e4m3 kernel: k-steps 4 / 8, 8 waves, 1 fragment
    ((1, 32, 2560, 2560, 5, 4), ((2, 1, 8, 4), (20, 5), 512, 16384)),
    ((1, 32, 2560, 2560, 5, 8), ((2, 1, 8, 8), (20, 5), 512, 16384)),
    ((1, 32, 2560, 2560, 5, 0x800), ((2, 1, 8, 4), (20, 5), 512, 16384)),
    ((1, 32, 2560, 2560, 5, 0x1000), ((2, 1, 8, 4), (20, 5), 512, 16384)),
    ((1, 32, 2560, 2560, 5, 16), ARG),
    ((1, 32, 2560, 2560, 5, 0x400), ARG),
    ((1, 32, 2560, 2560, 5, 0x2000), ARG),
    # the staged A slice within / beyond 150 KiB
    ((0, 64, 2560, 1184, 1, 0), ((4, 1, 8, 16), (20, 1), 512, 151552)),
    ((0, 64, 2560, 1216, 1, 0), SHAPE),
    ((1, 64, 2560, 2304, 1, 0), ((4, 1, 8, 8), (20, 1), 512, 147456)),
    ((1, 64, 2560, 2432, 1, 0), SHAPE),
    # what validate() says of a shape: ks must divide K / 32 (K / 128), M <= 64, ks >= 1
    ((0, 32, 128, 96, 2, 0), SHAPE),
    ((1, 32, 128, 192, 1, 0), SHAPE),
    ((0, 65, 128, 64, 1, 0), ARG),
    ((0, 32, 128, 64, 0, 0), ARG),
    ((0, 32, 128, 64, 0, 4), ARG),
    ((0, 64, 2560, 1216, 1, 4), SHAPE),                 # the slice before the selector
]

# (M, N, K, a_kind, gated, sel) -> ((16-row fragments, 16-column fragments, fp32 A, non-temporal weight loads), grid, 512, LDS bytes)
DIRECT = [
    # OPT-2.7B at M = 32: out-proj, QKV, FFN-up behind a LayerNorm on load and plain, FFN-down plain and behind a norm
    ((32, 2560, 2560, 0, 0, 0), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    ((32, 7680, 2560, 0, 0, 0), ((2, 2, 0, 1), (240, 1), 512, 41088)),
    ((32, 10240, 2560, 1, 0, 0), ((2, 3, 1, 1), (214, 1), 512, 59520)),
    ((32, 10240, 2560, 0, 0, 0), ((2, 3, 0, 1), (214, 1), 512, 59520)),
    ((32, 2560, 10240, 0, 0, 0), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    ((32, 2560, 10240, 1, 0, 0), ((2, 1, 1, 1), (160, 1), 512, 82432)),
    ((1, 64, 64, 0, 0, 0), ((1, 1, 0, 1), (4, 1), 512, 11328)),
    # 256 / 257 fragments of 16 columns
    ((32, 4096, 2560, 0, 0, 0), ((2, 1, 0, 1), (256, 1), 512, 22656)),
    ((32, 4112, 2560, 0, 0, 0), ((2, 2, 0, 1), (129, 1), 512, 41088)),
    # the caps: 4 fragments (2 at 64 rows); fp32 A: 3 fragments, and 33+ rows as two row groups of 32
    ((16, 16384, 2560, 0, 0, 0), ((1, 4, 0, 1), (256, 1), 512, 38976)),
    ((16, 50272, 2560, 0, 0, 0), ((1, 4, 0, 1), (786, 1), 512, 38976)),
    ((64, 50272, 2560, 0, 0, 0), ((4, 2, 0, 1), (1571, 1), 512, 82176)),
    ((32, 50272, 2560, 1, 0, 0), ((2, 3, 1, 1), (1048, 1), 512, 59520)),
    ((16, 50272, 2560, 2, 0, 0), ((1, 3, 1, 1), (1048, 1), 512, 29760)),
    ((64, 2560, 2560, 1, 0, 0), ((2, 1, 1, 1), (160, 2), 512, 22656)),
    ((64, 10240, 2560, 2, 0, 0), ((2, 3, 1, 1), (214, 2), 512, 59520)),
    ((33, 2560, 2560, 1, 0, 0), ((2, 1, 1, 1), (160, 2), 512, 22656)),
    # gated (both halves of a column in one workgroup): 256 / 320 fragments; the caps leave 2
    ((32, 4096, 2048, 0, 1, 0), ((2, 2, 0, 1), (256, 1), 512, 41088)),
    ((32, 5120, 2048, 0, 1, 0), ((2, 4, 0, 1), (160, 1), 512, 77952)),
    ((16, 5120, 2048, 0, 1, 0), ((1, 4, 0, 1), (160, 1), 512, 38976)),
    ((32, 5120, 2048, 2, 1, 0), ((2, 2, 1, 1), (320, 1), 512, 41088)),
    ((64, 5120, 2048, 0, 1, 0), ((4, 2, 0, 1), (320, 1), 512, 82176)),
    ((64, 5120, 2048, 2, 1, 0), ((2, 2, 1, 1), (320, 2), 512, 41088)),
    # fp32 A: gamma and beta in LDS up to K = 16384
    ((32, 2560, 16384, 1, 0, 0), ((2, 1, 1, 1), (160, 1), 512, 131584)),
    ((32, 2560, 16448, 1, 0, 0), ARG),
    ((32, 2560, 16448, 0, 0, 0), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    # sel: fragments 1..4 (5: no such kernel), plain weight loads, row groups, the bits that change no plan (ablations 0x20 / 0x40, rotate 0x80)
    ((32, 2560, 2560, 0, 0, 1), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    ((32, 2560, 2560, 0, 0, 2), ((2, 2, 0, 1), (80, 1), 512, 41088)),
    ((32, 2560, 2560, 0, 0, 3), ((2, 3, 0, 1), (54, 1), 512, 59520)),
    ((32, 2560, 2560, 0, 0, 4), ((2, 4, 0, 1), (40, 1), 512, 77952)),
    ((32, 2560, 2560, 0, 0, 5), SHAPE),
    ((32, 2560, 2560, 0, 0, 0x10), ((2, 1, 0, 0), (160, 1), 512, 22656)),
    ((32, 2560, 2560, 0, 0, 0x12), ((2, 2, 0, 0), (80, 1), 512, 41088)),
    ((32, 2560, 2560, 0, 0, 0x101), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    ((32, 2560, 2560, 0, 0, 0x201), ((1, 1, 0, 1), (160, 2), 512, 11328)),
    ((32, 2560, 2560, 0, 0, 0x400), ((1, 1, 0, 1), (160, 4), 512, 11328)),
    ((32, 2560, 2560, 0, 0, 0x20), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    ((32, 2560, 2560, 0, 0, 0x40), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    ((32, 2560, 2560, 0, 0, 0x80), ((2, 1, 0, 1), (160, 1), 512, 22656)),
    ((32, 2560, 2560, 0, 0, 0x82), ((2, 2, 0, 1), (80, 1), 512, 41088)),
    # 64 rows x 3 fragments: not instantiated; as two or four row groups they are
    ((64, 2560, 2560, 0, 0, 3), SHAPE),
    ((64, 2560, 2560, 0, 0, 0x203), ((2, 3, 0, 1), (54, 2), 512, 59520)),
    ((64, 2560, 2560, 0, 0, 0x404), ((1, 4, 0, 1), (40, 4), 512, 38976)),
    ((64, 2560, 2560, 1, 0, 3), ((2, 3, 1, 1), (54, 2), 512, 59520)),
    ((64, 2560, 2560, 1, 0, 0x103), SHAPE),             # fp32 A in ONE row group of 64
    ((64, 2560, 2560, 1, 0, 0x203), ((2, 3, 1, 1), (54, 2), 512, 59520)),
    ((64, 2560, 2560, 1, 0, 0x404), ((1, 4, 1, 1), (40, 4), 512, 38976)),
    ((32, 2560, 2560, 1, 0, 4), SHAPE),                 # fp32 A: 4 fragments at 16 rows only
    ((16, 2560, 2560, 1, 0, 4), ((1, 4, 1, 1), (40, 1), 512, 38976)),
    ((64, 2560, 2560, 0, 0, 0x101), ((4, 1, 0, 1), (160, 1), 512, 45312)),
    ((64, 2560, 2560, 0, 0, 0x301), ((2, 1, 0, 1), (160, 3), 512, 22656)),
    # the gate needs an even fragment count
    ((32, 5120, 2048, 0, 1, 3), ARG),
    ((32, 5120, 2048, 0, 1, 1), ARG),
    ((32, 5120, 2048, 0, 1, 4), ((2, 4, 0, 1), (160, 1), 512, 77952)),
    ((32, 5120, 2048, 0, 1, 2), ((2, 2, 0, 1), (320, 1), 512, 41088)),
    # what validate() says of a shape
    ((32, 2560, 96, 0, 0, 0), SHAPE),
    ((0, 64, 64, 0, 0, 0), ARG),
    ((65, 64, 64, 0, 0, 0), ARG),
    ((32, 64, 64, 3, 0, 0), DTYPE),
]

# the width of a statistics partial, eavqa_gemm_decode_cols(M, N, K, a_kind, gated): tests/test_decode_direct_gpu.py asserts the first four too
DECODE_COLS = [((32, 2560, 96, 0, 0), 0), ((32, 2560, 2560, 0, 0), 16), ((32, 7680, 2560, 0, 0), 32), ((32, 10240, 2560, 1, 0), 48),
               ((32, 5120, 2048, 0, 1), 32), ((32, 4096, 2048, 0, 1), 16), ((64, 50272, 2560, 0, 0), 32), ((65, 64, 64, 0, 0), 0)]

# (B, H, Sk, hd, path) -> ((lanes per key, waves per head, loads in flight, V mode), grid, workgroup, LDS bytes)
ATTENTION = [
    # OPT-2.7B (32 x 32 heads, 160 keys x 80): the LDS-image kernel.  T0-3B cross-attention (150 keys x 64): registers, 2 waves x 10 loads
    ((32, 32, 160, 80, 0), ((16, 4, 10, 1), (32, 8), 1024, 113152)),
    ((32, 32, 150, 64, 0), ((8, 2, 10, 2), (32, 8), 512, 6496)),
    # hd <= 64: one wave up to 80 keys, two up to 160, then the image
    ((32, 32, 1, 64, 0), ((8, 1, 10, 2), (32, 8), 256, 2064)),
    ((32, 32, 80, 64, 0), ((8, 1, 10, 2), (32, 8), 256, 3328)),
    ((32, 32, 81, 64, 0), ((8, 2, 10, 2), (32, 8), 512, 5392)),
    ((32, 32, 160, 64, 0), ((8, 2, 10, 2), (32, 8), 512, 6656)),
    ((32, 32, 161, 64, 0), ((8, 4, 10, 1), (32, 8), 1024, 93200)),
    # hd > 64: 40 / 80
    ((32, 32, 40, 80, 0), ((16, 1, 10, 2), (32, 8), 256, 2688)),
    ((32, 32, 41, 80, 0), ((16, 2, 10, 2), (32, 8), 512, 4752)),
    ((32, 32, 80, 80, 0), ((16, 2, 10, 2), (32, 8), 512, 5376)),
    ((32, 32, 81, 80, 0), ((16, 4, 10, 1), (32, 8), 1024, 61328)),
    # 256 / 257 and 512 / 513 workgroups (a last group of fewer than 4 heads counts)
    ((64, 16, 160, 80, 0), ((16, 4, 10, 1), (64, 4), 1024, 113152)),
    ((257, 4, 160, 80, 0), ((16, 2, 10, 0), (257, 1), 512, 6656)),
    ((64, 32, 160, 80, 0), ((16, 2, 10, 0), (64, 8), 512, 6656)),
    ((513, 4, 160, 80, 0), ((16, 1, 10, 0), (513, 1), 256, 4608)),
    ((32, 30, 160, 80, 0), ((16, 4, 10, 1), (32, 8), 1024, 113152)),
    ((32, 33, 160, 80, 0), ((16, 2, 10, 0), (32, 9), 512, 6656)),
    ((256, 4, 40, 64, 0), ((8, 1, 10, 2), (256, 1), 256, 2688)),
    ((257, 4, 40, 64, 0), ((8, 2, 10, 0), (257, 1), 512, 4736)),
    ((512, 4, 40, 64, 0), ((8, 2, 10, 0), (512, 1), 512, 4736)),
    ((513, 4, 40, 64, 0), ((8, 1, 10, 0), (513, 1), 256, 2688)),
    # the image has to fit 150 KiB with the scores: hd 16 at 1000 / 1024 keys; hd 128 at 139 / 140 keys and at the longest cache
    ((8, 32, 1000, 16, 0), ((8, 4, 10, 1), (8, 8), 1024, 152192)),
    ((8, 32, 1024, 16, 0), ((8, 4, 10, 0), (8, 8), 1024, 24576)),
    ((8, 20, 139, 128, 0), ((16, 4, 10, 1), (8, 5), 1024, 152752)),
    ((8, 20, 140, 128, 0), ((16, 4, 10, 0), (8, 5), 1024, 10432)),
    ((8, 20, 3584, 128, 0), ((16, 4, 10, 0), (8, 5), 1024, 65536)),
    # path bit 4: keep the LDS-image kernel; bit 5: registers up to 2 x 20 loads; both: bit 4 wins
    ((32, 32, 80, 64, 16), ((8, 4, 10, 1), (32, 8), 1024, 50432)),
    ((32, 32, 150, 64, 16), ((8, 4, 10, 1), (32, 8), 1024, 87392)),
    ((32, 32, 160, 80, 32), ((16, 2, 20, 2), (32, 8), 512, 6656)),
    ((32, 32, 161, 80, 32), ((16, 4, 10, 1), (32, 8), 1024, 113808)),
    ((32, 32, 320, 64, 32), ((8, 2, 20, 2), (32, 8), 512, 9216)),
    ((32, 32, 321, 64, 32), ((8, 4, 10, 0), (32, 8), 1024, 13328)),
    ((32, 32, 160, 80, 48), ((16, 4, 10, 1), (32, 8), 1024, 113152)),
    # outside the decode kernel's domain the decode forms are EAVQA_E_SHAPE (tests/test_abi.py: ATTENTION_REJECTIONS); the vector-ALU bit too
    ((32, 32, 160, 12, 0), SHAPE),
    ((32, 32, 160, 136, 0), SHAPE),
    ((32, 32, 3585, 80, 0), SHAPE),
    ((32, 32, 160, 80, 1), SHAPE),
    ((32, 32, 160, 6, 0), SHAPE),
    ((2048, 32, 160, 80, 0), SHAPE),                    # B H > 65535
    ((0, 32, 160, 80, 0), ARG),
]


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


def _route(lib, entry, row):
    from eavqa_amd import _lib
    plan = _lib.LaunchPlan()
    rc = getattr(lib, entry)(*row, C.byref(plan))
    return ((tuple(plan.variant), (plan.grid_x, plan.grid_y), plan.block, plan.lds_bytes) if rc == 0 else rc)


def _ids(table):
    return ["-".join(f"{v:x}" if i == len(r) - 1 else str(v) for i, v in enumerate(r)) + f"-{n}" for n, (r, _) in enumerate(table)]


@pytest.mark.parametrize("row,want", SPLITK, ids=_ids(SPLITK))
def test_splitk_plan_is_pinned(lib, row, want):
    assert _route(lib, "eavqa_gemm_splitk_route", row) == want


@pytest.mark.parametrize("row,want", DIRECT, ids=_ids(DIRECT))
def test_direct_plan_is_pinned(lib, row, want):
    assert _route(lib, "eavqa_gemm_decode_route", row) == want


@pytest.mark.parametrize("row,want", ATTENTION, ids=_ids(ATTENTION))
def test_decode_attention_plan_is_pinned(lib, row, want):
    assert _route(lib, "eavqa_attention_decode_route", row) == want


def test_decode_cols_is_the_plans_width(lib):
    assert [lib.eavqa_gemm_decode_cols(*row) for row, _ in DECODE_COLS] == [want for _, want in DECODE_COLS]
    for (M, N, K, a_kind, gated, sel), want in DIRECT:
        if sel == 0 and not isinstance(want, int):
            cols = lib.eavqa_gemm_decode_cols(M, N, K, a_kind, gated)
            assert cols == (8 if gated else 16) * want[0][1] and want[1][0] == -(-N // cols)


def test_a_null_plan_pointer_is_allowed_and_the_planned_split_is_legal(lib):
    assert lib.eavqa_gemm_splitk_route(0, 32, 2560, 2560, 10, 0, None) == 0
    assert lib.eavqa_gemm_decode_route(32, 2560, 2560, 0, 0, 0, None) == 0
    assert lib.eavqa_attention_decode_route(32, 32, 160, 80, 0, None) == 0
    for fp8, plan in ((0, lib.eavqa_gemm_splitk_plan), (1, lib.eavqa_gemm_fp8_splitk_plan)):
        for M, N, K in ((32, 7680, 2560), (1, 128, 128), (64, 50272, 2560), (17, 200, 384), (64, 12800, 512), (32, 2048, 5120)):
            assert lib.eavqa_gemm_splitk_route(fp8, M, N, K, plan(M, N, K), 0, None) == 0, (fp8, M, N, K)


def test_plan_properties_on_random_shapes(lib):
    """A few thousand pseudo-random shapes: a plan that is accepted names an instantiated variant, covers the problem with its grid and
    stays inside the LDS the kernels opt into."""
    import random
    rng = random.Random(20241)
    for _ in range(3000):
        fp8, M, N = rng.randint(0, 1), rng.randint(1, 64), rng.randint(1, 60000)
        ks = rng.randint(1, 12)
        K = ks * (128 if fp8 else 32) * rng.randint(1, 24)
        r = _route(lib, "eavqa_gemm_splitk_route", (fp8, M, N, K, ks, rng.choice((0, 0, rng.getrandbits(16)))))
        if not isinstance(r, int):
            (mf, nf, nw, u), (gx, gy), block, lds = r
            assert 16 * mf >= M and mf in (1, 2, 4) and block == 64 * nw and gy == ks and gx * 16 * nf * nw >= N > (gx - 1) * 16 * nf * nw
            assert lds == (K // ks) * 16 * mf * (1 if fp8 else 2) <= 150 * 1024
            assert (nf, nw) == (1, 8) and u in (4, 8) if fp8 else nf in (1, 2) and nw in (4, 8) and u in (8, 16)
        a_kind, gated = rng.choice((0, 0, 1, 2)), rng.randint(0, 1)
        K = 64 * rng.randint(1, 200)
        r = _route(lib, "eavqa_gemm_decode_route", (M, N, K, a_kind, gated, rng.choice((0, 0, rng.getrandbits(12)))))
        if not isinstance(r, int):
            (mf, nf, af32, nt), (gx, gy), block, lds = r
            cols = (8 if gated else 16) * nf
            assert 16 * mf * gy >= M and gx * cols >= N > (gx - 1) * cols and block == 512 and lds <= 150 * 1024 and af32 == (a_kind != 0)
            assert nf <= (2 if mf == 4 else 4) and (not af32 or (mf <= 2 and nf <= 3 + (mf == 1))) and (not gated or nf % 2 == 0)
        B, H, Sk, hd = rng.randint(1, 600), rng.randint(1, 40), rng.randint(1, 3584), 8 * rng.randint(1, 16)
        r = _route(lib, "eavqa_attention_decode_route", (B, H, Sk, hd, rng.choice((0, 0, 16, 32, 48))))
        if not isinstance(r, int):
            (lpk, wph, u, vmode), grid, block, lds = r
            assert lpk == (8 if hd <= 64 else 16) and grid == (B, (H + 3) // 4) and block == 256 * wph and lds <= 150 * 1024
            assert (wph, u, vmode) in ((1, 10, 2), (2, 10, 2), (2, 20, 2), (4, 10, 1), (4, 10, 0), (2, 10, 0), (1, 10, 0))
            assert lds == 16 * Sk + 2048 * wph + (8 * Sk * hd if vmode == 1 else 0)
