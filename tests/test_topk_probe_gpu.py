"""GPU: exact edge probes for ``eavqa_topk_rows`` and ``eavqa_l2_normalize_rows`` (csrc/retrieval.hip).

Top-k runs through ctypes so that the outputs are ``[rows + 1, k]`` buffers full of a sentinel (NaN / -7) whose surplus row must come
back untouched; every case runs on contiguous scores and on a ``[rows, cols + 5]`` window whose pad columns hold +inf, twice each
(bit-equal).  Reference: ``topk_reference`` of tests/_select_probe.py, a stable argsort on the kernel's documented key (-0 equal to
+0, NaNs with the sign clear above +inf, with the sign set below -inf, ties to the smaller column); indices ``array_equal``, values
as bit patterns.  What each case is: tests/test_select_probe_cpu.py.

Which case enters which path (and the mutation that turns it red; "run" = built into a scratch copy of the library and run on the
MI355X with the result stated; "read" = argued from the code):
  radix pass leaves by its own condition      test_topk_cases[bucket0_*], [all_minus_inf-*], [nans-*] and every row whose k-th key has a
                                              zero byte         `b > 0` -> `b > 1` (run: 36 of the 53 cases red, among them all of
                                              [bucket0_huge_negative-*], [all_minus_inf-*], [nans-*], [low_byte-*], [tie_cut-45],
                                              [bucket0_subnormals_zeros-1 / -150 / -200]; the l2 tests green)
  last radix byte                             test_topk_cases[low_byte*]: 256 keys that differ in the low byte only    (read)
  need_eq cut inside a later wave's segment   test_topk_cases[tie_cut-45], [all_equal-*], [grid_* row 2]: without the `pos < need_eq` test
                                              the kernel would write past cand[k] (moves an address: read, not run)
  cols below a wave / a segment, k == cols    test_topk_cases[grid_1-*] .. [grid_65-*]: the `c < c_end` guards, n2 = 1     (read)
  sort padding to the next power of two       test_topk_cases[grid_5000-1025], [grid_5000-2047]   (read)
  ld > cols                                   every case, window layout: a pad column read would win with +inf   (read)
  l2_normalize_kernel: tail of the column loop, window writes
                                              test_l2_normalize_window[*]: the buffer around the window is bit-unchanged (read)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _select_probe as P

DEV = "cuda"
CASES = [(name, k) for name, (x, ks) in P.topk_cases().items() for k in ks]


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import _lib
    lib = _lib.load()
    assert lib.eavqa_check_device() == 0, "not a gfx950 device"
    return lib


def _topk(lib, scores, cols, k):
    """``eavqa_topk_rows`` on a [rows, cols] window of ``scores``, into sentinel-filled buffers one row longer than needed"""
    rows = scores.shape[0]
    val = torch.full((rows + 1, k), math.nan, device=DEV)
    idx = torch.full((rows + 1, k), -7, device=DEV, dtype=torch.int64)
    rc = lib.eavqa_topk_rows(rows, cols, ctypes.c_void_p(scores.data_ptr()), scores.stride(0), k, ctypes.c_void_p(val.data_ptr()),
                             ctypes.c_void_p(idx.data_ptr()), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    assert np.isnan(val[rows]).all() and (val[rows].view(np.uint32) == np.float32(math.nan).view(np.uint32)).all() and (idx[rows] == -7).all()
    return val[:rows], idx[:rows]


@pytest.mark.parametrize("name,k", CASES, ids=[f"{n}-{k}" for n, k in CASES])
def test_topk_cases(lib, name, k):
    x, _ = P.topk_cases()[name]
    rows, cols = x.shape
    want_val, want_idx = P.topk_reference(x, k)
    window = np.full((rows, cols + 5), np.inf, np.float32)
    window[:, :cols] = x
    for what, scores in (("contiguous", torch.from_numpy(x).to(DEV)), ("window", torch.from_numpy(window).to(DEV))):
        val, idx = _topk(lib, scores, cols, k)
        assert np.array_equal(idx, want_idx), what
        assert P.same_bits(val, want_val).all(), what
        val2, idx2 = _topk(lib, scores, cols, k)
        assert np.array_equal(idx2, idx) and np.array_equal(val2.view(np.uint32), val.view(np.uint32)), what
        assert np.array_equal(scores.cpu().numpy().view(np.uint32), (x if what == "contiguous" else window).view(np.uint32)), what


L2_COLS = (1, 3, 255, 256, 257, 768, 1000)


def _l2(lib, x):
    """the rows of ``x`` normalised in place inside a [rows + 1, cols + 9] buffer full of 1e30, at column 3"""
    rows, cols = x.shape
    buf = torch.full((rows + 1, cols + 9), 1.0e30)
    buf[:rows, 3:3 + cols] = x
    dev = buf.to(DEV)
    view = dev[:rows, 3:3 + cols]
    rc = lib.eavqa_l2_normalize_rows(rows, cols, ctypes.c_void_p(view.data_ptr()), view.stride(0), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dev.cpu()
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[:rows, 3:3 + cols] = False
    assert torch.equal(got[outside].view(torch.int32), buf[outside].view(torch.int32))
    return got[:rows, 3:3 + cols]


@pytest.mark.parametrize("cols", L2_COLS)
def test_l2_normalize_window(lib, cols):
    """Per element within ``(ceil(cols / 256) + 16) 2^-24 |ref|`` of float64 ``x / ||x||``.  From the code: one rounding per square, at
    most ceil(cols / 256) - 1 sequential additions and 6 + 2 tree levels for the sum, all halved by the square root, then one rounding
    each for sqrt, reciprocal and product: ceil(cols / 256) / 2 + 7.5 units, the bound about twice that.  Everything outside the
    window must be bit-unchanged."""
    rows = 5
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(cols)) * torch.tensor([1.0, 1e-3, 50.0, 1.0, 7.0])[:, None]
    got = _l2(lib, x).double()
    ref = x.double() / x.double().norm(dim=1, keepdim=True)
    bound = (math.ceil(cols / 256) + 16) * 2.0 ** -24 * ref.abs()
    err = (got - ref).abs()
    print(f"[cols {cols}] max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert (err <= bound).all()


def test_l2_normalize_rows_whose_norm_is_zero_or_infinite(lib):
    """The contract: a row is divided by the float32 square root of its float32 sum of squares.  A zero row stays zero bit for bit; a
    row of 1e-30 is left alone (its squares underflow to 0, the norm is 0: faiss's rule as well); a row holding 3e20 becomes zeros
    (the sum of squares is +inf, so 1 / sqrt is 0)."""
    cols = 300
    x = torch.randn(4, cols, generator=torch.Generator().manual_seed(2))
    x[0] = 0.0
    x[0, 5] = -0.0
    x[1] = 1e-30
    x[2, 17] = 3e20
    got = _l2(lib, x)
    assert torch.equal(got[0].view(torch.int32), x[0].view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), x[1].view(torch.int32))
    assert (got[2] == 0).all()
    ref = x[3].double() / x[3].double().norm()
    assert ((got[3].double() - ref).abs() <= (math.ceil(cols / 256) + 16) * 2.0 ** -24 * ref.abs()).all()
