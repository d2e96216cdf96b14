"""GPU: exact probes of the row-wise e4m3 quantiser (eavqa_quantize_rows_fp8: the generic and the register kernel at the end of
csrc/gemm_fp8.hip) against the float64 reference of tests/_fp8_ref.py, whose header states the contract (``check_row``) and which
tests/test_fp8_ref_cpu.py pins to torch's float8_e4m3fn.  The fused twins (eavqa_layernorm_fwd_fp8 / _bwd_fp8 / _splitk_fp8) are held to the
same ``check_row`` in tests/test_fp8_gpu.py.

Every call writes into slices of larger buffers (bytes 0xA5, scales NaN, one surplus row and surplus columns: the surplus must come back
untouched) and reads a column slice of a wider matrix whose other entries are 3e38 (a read outside the slice shows in the row's amax).
Base pointers keep the alignment of the loads the kernel issues: 16 bytes for f32 rows and for the register kernel, 8 for the generic
kernel's bf16 rows.

Which case enters which path is the table PATH_CASES of tests/_fp8_ref.py (test_path_table_is_the_dispatch there restates the dispatch of
csrc/gemm.hip).  The row maximum is planted in turn at the first column, the last, a column the block's last wave owns in the first pass
and a column of the second pass, negative in every third row.

Mutations (each changes values only, never an address or a bound; "run": built into a scratch copy of the library and run on the MI355X
against this file; the CPU mirror of the same mutation is flagged on the same case by test_each_value_mutant_is_flagged_on_its_case):
  generic kernel's amax loop stops after its first pass (`c < cols && c < 1024`)
        test_every_path...[generic-{f32,bf16}-{1028,2052}-*], [generic-bf16-16392-*] red (the maximum in the second pass); every single-pass
        case and every register-kernel case green (run)
  red[3] left out of the block combine (both kernels)
        test_every_path...[generic-*] from 1020 columns up and [reg-bf16-*] from 2048 up red (the maximum in the last wave's share);
        [generic-*-4], [generic-bf16-12], [reg-bf16-8] green: their rows end before that wave's share (run)
  register kernel's amax skips element 7 of each vector (`e < 7`)
        test_every_path...[reg-bf16-*], all sixteen, red (the maximum in the last column); every generic case green (run)
  the two cvt_pk word selects swapped (bytes 2 3 0 1 of every four)
        every case of this file red (run)
  the scale floor removed (the code before this file existed)
        test_tiny_rows_get_finite_bytes[*], test_subnormal_inputs_stay_finite[*], test_tiny_row_through_the_fp8_gemm and, in
        tests/test_fp8_gpu.py, test_layernorm_bwd_fp8_on_tiny_gradient_rows[*] red: NaN bytes, scales below 2^-126; all else green (run)
  row_scale[row] written from the unreduced amax of thread 0
        test_every_path... red wherever a row is longer than thread 0's share ([generic-*] from 12 columns up, [reg-bf16-*] from 2048
        up), the tie rows, the sweep through the generic kernel, the poisoned rows and the consumer test red (run)
The older tests of tests/test_fp8_gpu.py turned red with the mutants as well (they compare with a mirror of the same arithmetic, and the
fused twins with this kernel); what they could not see is the floor: their mirror overflowed with the kernel.

Subnormal inputs: the MI355X keeps them - test_subnormal_inputs_stay_finite read back encode(x * 2^126) for every fp32- and bf16-subnormal
element (0x30 for 2^-127, 0x04 for 2^-133), from both kernels; the test asserts only what also holds on a device that reads them as zeros.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _fp8_ref as R

DEV = "cuda"
POISON = 3e38


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


def quantize_guarded(ops, x, shape):
    """One call on ``x`` [rows, cols] laid out as ``shape`` (a row of PATH_CASES / VALUE_SHAPES) says: x a column slice of a wider matrix
    of 3e38, the outputs slices of guard buffers.  Returns (bytes, scales) as numpy arrays after asserting that nothing outside the
    slices was written and that the base pointers have the alignment the case promises."""
    _, kernel, dtype, cols, ldx, cx, ld_out, co = shape
    rows = x.shape[0]
    assert x.shape == (rows, cols) and x.dtype == dtype
    wide = torch.full((rows, ldx), POISON, dtype=dtype)
    wide[:, cx:cx + cols] = x
    xs = wide.to(DEV)[:, cx:cx + cols]
    qbuf = torch.full((rows + 1, ld_out), 0xA5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((rows + 5,), float("nan"), dtype=torch.float32, device=DEV)
    q, sc = qbuf[:rows, co:co + cols], sbuf[2:2 + rows]
    assert xs.data_ptr() % (16 if dtype == R.F32 or kernel == "reg" else 8) == 0 and q.data_ptr() % (8 if kernel == "reg" else 4) == 0
    got = ops.quantize_rows_fp8(xs, out=q, scale_out=sc)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == q.data_ptr() and got[1].data_ptr() == sc.data_ptr()
    qb, sb = qbuf.cpu(), sbuf.cpu()
    outside = torch.ones(qb.shape, dtype=torch.bool)
    outside[:rows, co:co + cols] = False
    assert bool((qb[outside] == 0xA5).all()), "bytes outside the output slice were written"
    assert bool(torch.isnan(sb[:2]).all()) and bool(torch.isnan(sb[2 + rows:]).all()), "scales outside the output slice were written"
    return qb[:rows, co:co + cols].numpy().copy(), sb[2:2 + rows].numpy().copy()


def conforms(x, q, sc, allow, stats=None):
    bad = R.check_rows(R.f64(x), q, sc, allow=allow, stats=stats)
    assert not bad, "\n".join(bad[:8])


# ================================================================================================== paths, strides, guards, the amax
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("case", R.PATH_CASES, ids=[c[0] for c in R.PATH_CASES])
def test_every_path_with_strides_and_guards(ops, case, rows):
    stats = {}
    for turn in range(4):
        x = R.path_input(case, rows, turn)
        q, sc = quantize_guarded(ops, x, case)
        conforms(x, q, sc, True, stats)
        assert sc.tolist() == [R.contract_scale(R.PLANT)] * rows
    assert stats["allowed"] <= R.MAX_TIE_SHARE * stats["elements"]


# ============================================================================================================ value tables
SHAPES = pytest.mark.parametrize("shape", R.VALUE_SHAPES, ids=[s[0] for s in R.VALUE_SHAPES])


@SHAPES
@pytest.mark.parametrize("k", R.TIE_EXPONENTS)
def test_tie_rows_are_exact(ops, shape, k):
    """amax = 448 * 2^k: the scale is 2^k and every quotient exact, so every midpoint goes to its even code, one fp32 ulp beside it to that
    side's code, the zeros keep their signs - bytes and scale equal the reference's, no allowance."""
    x = R.tie_row(k, shape[2], shape[3])
    q, sc = quantize_guarded(ops, x, shape)
    want, scale = R.spec(R.f64(x))
    assert sc.tolist() == [2.0 ** k] == scale.tolist()
    assert np.array_equal(q, want), np.flatnonzero(q[0] != want[0])[:8]
    conforms(x, q, sc, False)


@SHAPES
def test_magnitude_sweep(ops, shape):
    """Gaussian rows times 2^-110 .. 2^110 and a row whose amax is the largest finite value of the type."""
    x = R.sweep_rows(shape[2], shape[3])
    q, sc = quantize_guarded(ops, x, shape)
    stats = {}
    conforms(x, q, sc, True, stats)
    assert stats["allowed"] <= R.MAX_TIE_SHARE * stats["elements"]
    assert np.isfinite(sc).all() and sc[-1] == np.float32(torch.finfo(shape[2]).max) * R.INV448_F32


@SHAPES
def test_tiny_rows_get_finite_bytes(ops, shape):
    """Rows below the floor (0 < amax < 448 * 2^-126): scale 2^-126, bytes encode(x * 2^126) exactly.  Before the floor the reciprocal of
    amax / 448 overflowed and every element - the exact zeros too - left as a NaN byte."""
    x = R.tiny_rows(shape[2], shape[3])
    q, sc = quantize_guarded(ops, x, shape)
    assert not ((q & 0x7F) == 0x7F).any(), "NaN bytes in a finite row"
    assert sc.tolist() == [R.FLOOR, R.FLOOR]
    assert np.array_equal(q[0], R.e4m3_encode(np.arange(shape[3]) % 7 - 3.0))
    assert np.array_equal(q[1], R.e4m3_encode(np.ldexp(R.f64(x)[1], 126)))
    conforms(x, q, sc, False)


@SHAPES
def test_first_row_the_floor_does_not_touch(ops, shape):
    """amax = 448 * 2^-126 exactly: scale 2^-126 from the product itself, every tie of magnitude >= 1 exact."""
    x = R.first_unfloored_row(shape[2], shape[3])
    q, sc = quantize_guarded(ops, x, shape)
    assert sc.tolist() == [R.FLOOR] and np.array_equal(q, R.spec(R.f64(x))[0])
    conforms(x, q, sc, False)


@SHAPES
def test_subnormal_inputs_stay_finite(ops, shape):
    """fp32-subnormal elements under a normal maximum: no NaN byte, scale 2^-126, |dequantised - x| <= 2^-126 - true whether or not the
    device reads a subnormal input as zero (which of the two it does is printed, and recorded in the header)."""
    x = R.subnormal_row(shape[2], shape[3])
    q, sc = quantize_guarded(ops, x, shape)
    assert not ((q & 0x7F) == 0x7F).any() and sc.tolist() == [R.FLOOR]
    back = R.e4m3_decode(q) * R.FLOOR
    assert (np.abs(back - R.f64(x)) <= R.FLOOR).all()
    kept = np.array_equal(q, R.e4m3_encode(np.ldexp(R.f64(x), 126)))
    print(f"[{shape[0]}] subnormal inputs: first eight bytes {[hex(b) for b in q[0, :8]]} - {'kept (x * 2^126 encoded exactly)' if kept else 'NOT all kept'}")


@SHAPES
@pytest.mark.parametrize("last", [False, True], ids=["first-column", "last-column"])
def test_poisoned_rows_stay_poisoned_and_alone(ops, shape, last):
    """A NaN, a +inf, a -inf, each in its own row: the element dequantises to a non-finite number, and every other row of the call is
    bit-equal - bytes and scale - to the call with the poisoned rows replaced by zeros."""
    x, clean = R.poisoned_rows(shape[2], shape[3], last)
    q, sc = quantize_guarded(ops, x, shape)
    qc, scc = quantize_guarded(ops, clean, shape)
    conforms(x, q, sc, True)
    conforms(clean, qc, scc, True)
    col = shape[3] - 1 if last else 0
    with np.errstate(all="ignore"):
        for r in R.POISONED:
            assert not np.isfinite(R.e4m3_decode(q[r, col]) * np.float64(sc[r]))
            assert scc[r] == 1.0 and not qc[r].any()
    for r in range(5):
        if r not in R.POISONED:
            assert np.array_equal(q[r], qc[r]) and sc[r].tobytes() == scc[r].tobytes()


# ======================================================================================================= through the consumer
def test_tiny_row_through_the_fp8_gemm(ops):
    """quantize_rows_fp8 -> gemm_fp8 (b_scale 1) on integer-valued B: row 0 small integers whose maximum 7 = 448 / 64 makes the scale 2^-6
    and every quotient a code, row 1 the tiny row 2^-126 * n, row 2 zeros.  All exact, so the fp32 output equals x @ B^T; every nonzero
    entry of row 1 is an integer times 2^-126 - a normal fp32."""
    M, N, K = 3, 64, 128
    g = torch.Generator().manual_seed(4)
    x = torch.zeros(M, K)
    x[0] = torch.randint(-7, 8, (K,), generator=g).float()
    x[0, 17] = 7.0
    x[1] = (torch.arange(K) % 7 - 3).double().mul(R.FLOOR).float()
    b = torch.randint(-2, 3, (N, K), generator=g).float()
    b[:, 5::11] = (torch.arange(N)[:, None] % 4).float() - 2
    xq, xs = ops.quantize_rows_fp8(x.to(DEV))
    bq = torch.from_numpy(R.e4m3_encode(b.double().numpy())).to(DEV)
    out = ops.gemm_fp8(xq, xs, bq, 1.0, out_f32=True).cpu()
    assert xs.cpu().tolist() == [2.0 ** -6, R.FLOOR, 1.0]
    want = (x.double() @ b.double().T).float()
    assert torch.equal(want.double(), x.double() @ b.double().T)                 # the expected product is itself an fp32 matrix
    assert torch.equal(out, want)
    nz = out[1][out[1] != 0]
    assert len(nz) > N // 2 and bool((nz.abs() >= R.FLOOR).all()) and not bool(out[2].any())
