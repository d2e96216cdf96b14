"""Host only: the status code of every normalisation entry point for calls it rejects BEFORE any HIP call (validate() of
csrc/norm_params.h).  The codes, and which check wins when two fail, were read off the entry points as they stood before the family
got one host layer.  The pointers are small integers, not buffers: a validation bug must show as a wrong code on a machine without a
GPU, never as a launch on one - so the module skips itself where a GPU is present."""
import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("the calls carry made-up pointers: host-only machines only", allow_module_level=True)

ARG, ALIGN, SHAPE, DTYPE = -1, -2, -3, -4          # EAVQA_E_* (asserted against the header below)
F32, BF16, F16 = 0, 1, 2
P = 4096                                           # a non-NULL "pointer"

# a call every check accepts, per entry point (parameter names as include/eavqa.h declares them)
GOOD = {
    "eavqa_layernorm_fwd": dict(dtype=BF16, x_kind=0, rows=2, cols=8, x=P, ldx=8, gamma=P, beta=P, eps=1e-5, y=P, ldy=8, mean=P, rstd=P, stream=None),
    "eavqa_layernorm_fwd_fp8": dict(x_kind=2, rows=2, cols=8, x=P, ldx=8, gamma=P, beta=P, eps=1e-5, yq=P, ldq=8, row_scale=P, mean=P, rstd=P, stream=None),
    "eavqa_layernorm_bwd": dict(dtype=BF16, x_f32=0, rows=2, cols=8, x=P, ldx=8, dy=P, lddy=8, gamma=P, mean=P, rstd=P, dres=P, dx=P, lddx=8,
                                dgamma=None, dbeta=None, dx_lowp=P, ld_lowp=8, stream=None),
    "eavqa_layernorm_bwd_fp8": dict(x_f32=0, rows=2, cols=8, x=P, ldx=8, dy=P, lddy=8, gamma=P, mean=P, rstd=P, dres=P, dx=P, lddx=8, dxq=P, ldq=8,
                                    row_scale=P, stream=None),
    "eavqa_rmsnorm_fwd": dict(dtype=BF16, x_kind=0, rows=2, cols=8, x=P, ldx=8, gamma=P, eps=1e-6, y=P, ldy=8, rstd=P, stream=None),
    "eavqa_rmsnorm_bwd": dict(dtype=BF16, x_kind=0, rows=2, cols=8, x=P, ldx=8, dy=P, lddy=8, gamma=P, rstd=P, dres=P, dx=P, lddx=8, dx_lowp=P, ld_lowp=8,
                              stream=None),
    "eavqa_layernorm_splitk": dict(dtype=BF16, rows=2, cols=8, x_in=P, ldx=8, partials=P, ks=2, bias=P, x_out=P, ld_out=8, gamma=P, beta=P, eps=1e-5,
                                   y=P, ldy=8, stream=None),
    "eavqa_layernorm_splitk_fp8": dict(rows=2, cols=8, x_in=P, ldx=8, partials=P, ks=2, bias=P, x_out=P, ld_out=8, gamma=P, beta=P, eps=1e-5, yq=P, ldq=8,
                                       row_scale=P, stream=None),
    "eavqa_rmsnorm_splitk": dict(dtype=BF16, rows=2, cols=8, x_in=P, ldx=8, partials=P, ks=2, x_out=P, ld_out=8, gamma=P, eps=1e-6, y=P, ldy=8, stream=None),
}

# (entry point, what the call changes in GOOD, status code)
TABLE = [
    # ---- eavqa_layernorm_fwd: arguments, shape (cols % 4, cols <= 8192), alignment, x_kind, dtype
    ("eavqa_layernorm_fwd", dict(x=None), ARG),
    ("eavqa_layernorm_fwd", dict(y=None), ARG),
    ("eavqa_layernorm_fwd", dict(rows=0), ARG),
    ("eavqa_layernorm_fwd", dict(cols=0), ARG),
    ("eavqa_layernorm_fwd", dict(cols=6), SHAPE),
    ("eavqa_layernorm_fwd", dict(cols=8196, ldx=8196, ldy=8196), SHAPE),
    ("eavqa_layernorm_fwd", dict(ldx=10), ALIGN),
    ("eavqa_layernorm_fwd", dict(ldy=10), ALIGN),
    ("eavqa_layernorm_fwd", dict(x_kind=4), DTYPE),
    ("eavqa_layernorm_fwd", dict(x_kind=-1), DTYPE),
    ("eavqa_layernorm_fwd", dict(dtype=3), DTYPE),
    ("eavqa_layernorm_fwd", dict(rows=0, cols=6), ARG),
    ("eavqa_layernorm_fwd", dict(cols=6, ldx=10), SHAPE),
    ("eavqa_layernorm_fwd", dict(ldx=10, x_kind=4, dtype=3), ALIGN),
    # ---- eavqa_layernorm_fwd_fp8: the bytes and the scales are required; x_kind 0 has no dtype to mean
    ("eavqa_layernorm_fwd_fp8", dict(x=None), ARG),
    ("eavqa_layernorm_fwd_fp8", dict(yq=None), ARG),
    ("eavqa_layernorm_fwd_fp8", dict(row_scale=None), ARG),
    ("eavqa_layernorm_fwd_fp8", dict(rows=0), ARG),
    ("eavqa_layernorm_fwd_fp8", dict(cols=6), SHAPE),
    ("eavqa_layernorm_fwd_fp8", dict(cols=8196, ldx=8196, ldq=8196), SHAPE),
    ("eavqa_layernorm_fwd_fp8", dict(ldx=10), ALIGN),
    ("eavqa_layernorm_fwd_fp8", dict(ldq=10), ALIGN),
    ("eavqa_layernorm_fwd_fp8", dict(x_kind=0), DTYPE),
    ("eavqa_layernorm_fwd_fp8", dict(x_kind=4), DTYPE),
    ("eavqa_layernorm_fwd_fp8", dict(ldq=10, x_kind=0), ALIGN),
    # ---- eavqa_layernorm_bwd: bfloat16 / float32 only; the 4096-column limit is the LAST check
    ("eavqa_layernorm_bwd", dict(x=None), ARG),
    ("eavqa_layernorm_bwd", dict(dy=None), ARG),
    ("eavqa_layernorm_bwd", dict(dx=None), ARG),
    ("eavqa_layernorm_bwd", dict(mean=None), ARG),
    ("eavqa_layernorm_bwd", dict(rstd=None), ARG),
    ("eavqa_layernorm_bwd", dict(rows=0), ARG),
    ("eavqa_layernorm_bwd", dict(cols=6), SHAPE),
    ("eavqa_layernorm_bwd", dict(cols=4100, ldx=4100, lddy=4100, lddx=4100, ld_lowp=4100), SHAPE),
    ("eavqa_layernorm_bwd", dict(ldx=10), ALIGN),
    ("eavqa_layernorm_bwd", dict(lddy=10), ALIGN),
    ("eavqa_layernorm_bwd", dict(lddx=10), ALIGN),
    ("eavqa_layernorm_bwd", dict(ld_lowp=10), ALIGN),
    ("eavqa_layernorm_bwd", dict(dtype=F16), DTYPE),
    ("eavqa_layernorm_bwd", dict(dtype=3), DTYPE),
    ("eavqa_layernorm_bwd", dict(cols=4100, dtype=F16), DTYPE),
    ("eavqa_layernorm_bwd", dict(cols=4100, ldx=10), ALIGN),
    ("eavqa_layernorm_bwd", dict(dx=None, cols=6), ARG),
    # x_f32 is a flag.  (Not a rejection of old: 2 / 3 used to reach the row kernel as bfloat16 / half while ln_dparam_kernel read float32.)
    ("eavqa_layernorm_bwd", dict(x_f32=2), DTYPE),          # (bfloat16 storage; float32 storage ignores x_f32 as it always has)
    ("eavqa_layernorm_bwd_fp8", dict(x_f32=2), DTYPE),
    # ---- eavqa_layernorm_bwd_fp8
    ("eavqa_layernorm_bwd_fp8", dict(x=None), ARG),
    ("eavqa_layernorm_bwd_fp8", dict(mean=None), ARG),
    ("eavqa_layernorm_bwd_fp8", dict(dxq=None), ARG),
    ("eavqa_layernorm_bwd_fp8", dict(row_scale=None), ARG),
    ("eavqa_layernorm_bwd_fp8", dict(rows=0), ARG),
    ("eavqa_layernorm_bwd_fp8", dict(cols=6), SHAPE),
    ("eavqa_layernorm_bwd_fp8", dict(cols=4100, ldx=4100, lddy=4100, lddx=4100, ldq=4100), SHAPE),
    ("eavqa_layernorm_bwd_fp8", dict(lddy=10), ALIGN),
    ("eavqa_layernorm_bwd_fp8", dict(ldq=10), ALIGN),
    ("eavqa_layernorm_bwd_fp8", dict(cols=4100, ldq=10), ALIGN),
    # ---- eavqa_rmsnorm_fwd: no half
    ("eavqa_rmsnorm_fwd", dict(x=None), ARG),
    ("eavqa_rmsnorm_fwd", dict(y=None), ARG),
    ("eavqa_rmsnorm_fwd", dict(rows=0), ARG),
    ("eavqa_rmsnorm_fwd", dict(cols=6), SHAPE),
    ("eavqa_rmsnorm_fwd", dict(cols=8196, ldx=8196, ldy=8196), SHAPE),
    ("eavqa_rmsnorm_fwd", dict(ldy=10), ALIGN),
    ("eavqa_rmsnorm_fwd", dict(x_kind=4), DTYPE),
    ("eavqa_rmsnorm_fwd", dict(dtype=F16), DTYPE),
    # ---- eavqa_rmsnorm_bwd: no mean; x_kind and dtype before the 4096-column limit
    ("eavqa_rmsnorm_bwd", dict(x=None), ARG),
    ("eavqa_rmsnorm_bwd", dict(dy=None), ARG),
    ("eavqa_rmsnorm_bwd", dict(dx=None), ARG),
    ("eavqa_rmsnorm_bwd", dict(rstd=None), ARG),
    ("eavqa_rmsnorm_bwd", dict(rows=0), ARG),
    ("eavqa_rmsnorm_bwd", dict(cols=6), SHAPE),
    ("eavqa_rmsnorm_bwd", dict(cols=4100, ldx=4100, lddy=4100, lddx=4100, ld_lowp=4100), SHAPE),
    ("eavqa_rmsnorm_bwd", dict(lddx=10), ALIGN),
    ("eavqa_rmsnorm_bwd", dict(ld_lowp=10), ALIGN),
    ("eavqa_rmsnorm_bwd", dict(x_kind=4), DTYPE),
    ("eavqa_rmsnorm_bwd", dict(x_kind=-1), DTYPE),
    ("eavqa_rmsnorm_bwd", dict(dtype=F16), DTYPE),
    ("eavqa_rmsnorm_bwd", dict(cols=4100, x_kind=4), DTYPE),
    ("eavqa_rmsnorm_bwd", dict(lddx=10, x_kind=4), ALIGN),
    # ---- eavqa_layernorm_splitk: beta, then the dtype, then the other arguments; cols <= 16384
    ("eavqa_layernorm_splitk", dict(beta=None), ARG),
    ("eavqa_layernorm_splitk", dict(beta=None, dtype=F16), ARG),
    ("eavqa_layernorm_splitk", dict(dtype=F16), DTYPE),
    ("eavqa_layernorm_splitk", dict(dtype=F16, x_in=None), DTYPE),
    ("eavqa_layernorm_splitk", dict(x_in=None), ARG),
    ("eavqa_layernorm_splitk", dict(gamma=None), ARG),
    ("eavqa_layernorm_splitk", dict(y=None), ARG),
    ("eavqa_layernorm_splitk", dict(rows=0), ARG),
    ("eavqa_layernorm_splitk", dict(ks=-1), ARG),
    ("eavqa_layernorm_splitk", dict(partials=None), ARG),
    ("eavqa_layernorm_splitk", dict(cols=6), SHAPE),
    ("eavqa_layernorm_splitk", dict(cols=16388, ldx=16388, ld_out=16388, ldy=16388), SHAPE),
    ("eavqa_layernorm_splitk", dict(ldx=10), ALIGN),
    ("eavqa_layernorm_splitk", dict(ldy=10), ALIGN),
    ("eavqa_layernorm_splitk", dict(ld_out=10), ALIGN),
    ("eavqa_layernorm_splitk", dict(cols=6, ldx=10), SHAPE),
    # ---- eavqa_layernorm_splitk_fp8: a missing scale pointer and an unaligned ldq are argument errors here
    ("eavqa_layernorm_splitk_fp8", dict(beta=None), ARG),
    ("eavqa_layernorm_splitk_fp8", dict(yq=None), ARG),
    ("eavqa_layernorm_splitk_fp8", dict(row_scale=None), ARG),
    ("eavqa_layernorm_splitk_fp8", dict(ldq=10), ARG),
    ("eavqa_layernorm_splitk_fp8", dict(x_in=None), ARG),
    ("eavqa_layernorm_splitk_fp8", dict(cols=6), SHAPE),
    ("eavqa_layernorm_splitk_fp8", dict(cols=16388, ldx=16388, ld_out=16388, ldq=16388), SHAPE),
    ("eavqa_layernorm_splitk_fp8", dict(ld_out=10), ALIGN),
    # ---- eavqa_rmsnorm_splitk
    ("eavqa_rmsnorm_splitk", dict(dtype=F16), DTYPE),
    ("eavqa_rmsnorm_splitk", dict(dtype=F16, gamma=None), DTYPE),
    ("eavqa_rmsnorm_splitk", dict(gamma=None), ARG),
    ("eavqa_rmsnorm_splitk", dict(y=None), ARG),
    ("eavqa_rmsnorm_splitk", dict(rows=0), ARG),
    ("eavqa_rmsnorm_splitk", dict(partials=None), ARG),
    ("eavqa_rmsnorm_splitk", dict(cols=6), SHAPE),
    ("eavqa_rmsnorm_splitk", dict(cols=16388, ldx=16388, ld_out=16388, ldy=16388), SHAPE),
    ("eavqa_rmsnorm_splitk", dict(ldy=10), ALIGN),
]


def test_codes_are_the_headers():
    from eavqa_amd import _lib
    got = tuple(_lib.CONSTANTS[n] for n in ("EAVQA_E_ARG", "EAVQA_E_ALIGN", "EAVQA_E_SHAPE", "EAVQA_E_DTYPE", "EAVQA_F32", "EAVQA_BF16", "EAVQA_F16"))
    assert got == (ARG, ALIGN, SHAPE, DTYPE, F32, BF16, F16)
    assert set(GOOD) == {n for n in _lib.SIGNATURES if "norm" in n and (n.startswith("eavqa_layernorm") or n.startswith("eavqa_rmsnorm"))}


def test_rejected_calls_return_their_code():
    from eavqa_amd import _lib
    lib = _lib.load()
    failed = []
    for entry, change, want in TABLE:
        assert set(change) <= set(GOOD[entry]), (entry, change)
        args = dict(GOOD[entry], **change)
        assert list(args) == list(_lib.PARAMS[entry]), f"{entry}: GOOD does not follow the header's parameter order"
        got = getattr(lib, entry)(*args.values())
        if got != want:
            failed.append(f"{entry}({change}) returned {got}, want {want}")
    assert not failed, "\n".join(failed)
