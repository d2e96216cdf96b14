"""Host only: the status code of eavqa_quantize_rows_fp8 for calls it rejects BEFORE any HIP call (csrc/gemm.hip), as the entry point answers
today, and which check wins when two fail.  Same form as tests/test_norm_reject_cpu.py: the pointers are small integers, not buffers - a
validation bug must show as a wrong code on a machine without a GPU, never as a launch on one - so the module skips itself where a GPU is
present."""
import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("the calls carry made-up pointers: host-only machines only", allow_module_level=True)

ARG, ALIGN, SHAPE, DTYPE = -1, -2, -3, -4          # EAVQA_E_* (asserted against the header below)
F32, BF16, F16 = 0, 1, 2
P = 4096                                           # a non-NULL "pointer"
ENTRY = "eavqa_quantize_rows_fp8"

# a call every check accepts (parameter names as include/eavqa.h declares them)
GOOD = dict(dtype=BF16, rows=2, cols=8, x=P, ldx=8, out=P, ld_out=8, row_scale=P, stream=None)

# (what the call changes in GOOD, status code): arguments, shape (cols % 4), leading dimensions, base pointers (x 8 bytes, out 4), dtype
TABLE = [
    (dict(x=None), ARG),
    (dict(out=None), ARG),
    (dict(row_scale=None), ARG),
    (dict(rows=0), ARG),
    (dict(rows=-1), ARG),
    (dict(cols=0), ARG),
    (dict(cols=-4), ARG),
    (dict(cols=6), SHAPE),
    (dict(cols=2, ldx=4, ld_out=4), SHAPE),
    (dict(ldx=4), ALIGN),                          # below cols
    (dict(ld_out=4), ALIGN),
    (dict(ldx=10), ALIGN),                         # no multiple of 4
    (dict(ld_out=10), ALIGN),
    (dict(x=P + 4), ALIGN),
    (dict(x=P + 2), ALIGN),
    (dict(out=P + 2), ALIGN),
    (dict(out=P + 1), ALIGN),
    (dict(dtype=F32, x=P + 4), ALIGN),             # the 8-byte rule does not depend on the type
    (dict(dtype=F16), DTYPE),
    (dict(dtype=3), DTYPE),
    (dict(dtype=-1), DTYPE),
    # two at once: arguments, then the shape, then the leading dimensions and the pointers, the dtype last
    (dict(x=None, cols=6), ARG),
    (dict(rows=0, dtype=3), ARG),
    (dict(cols=6, ldx=10), SHAPE),
    (dict(cols=6, x=P + 4), SHAPE),
    (dict(cols=6, dtype=3), SHAPE),
    (dict(ldx=10, dtype=3), ALIGN),
    (dict(ld_out=4, x=P + 4), ALIGN),
    (dict(out=P + 2, dtype=3), ALIGN),
]


def test_codes_are_the_headers():
    from eavqa_amd import _lib
    got = tuple(_lib.CONSTANTS[n] for n in ("EAVQA_E_ARG", "EAVQA_E_ALIGN", "EAVQA_E_SHAPE", "EAVQA_E_DTYPE", "EAVQA_F32", "EAVQA_BF16", "EAVQA_F16"))
    assert got == (ARG, ALIGN, SHAPE, DTYPE, F32, BF16, F16)
    assert list(GOOD) == list(_lib.PARAMS[ENTRY]), "GOOD does not follow the header's parameter order"


def test_rejected_calls_return_their_code():
    from eavqa_amd import _lib
    lib = _lib.load()
    failed = []
    for change, want in TABLE:
        assert set(change) <= set(GOOD), change
        assert want != 0
        got = getattr(lib, ENTRY)(*dict(GOOD, **change).values())
        if got != want:
            failed.append(f"{ENTRY}({change}) returned {got}, want {want}")
    assert not failed, "\n".join(failed)
