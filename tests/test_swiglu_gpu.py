"""GPU: eavqa_swiglu_fwd / _bwd / _splitk (csrc/llama.hip) against float64 torch, at the tolerances tests/test_t5_gpu.py holds
eavqa_gated_act_fwd / _bwd (float32 1e-5, bfloat16 3e-2) and eavqa_splitk_finish_gated (2e-5, 2e-2) to, relative to max(1, max |ref|)."""
import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("F", [32, 160])
def test_swiglu_forward_backward(ops, dtype, rows, F):
    u = rnd(rows, 2 * F, seed=1, dtype=dtype, scale=2.0)
    dh = rnd(rows, F, seed=2, dtype=dtype)
    uu = u.double().clone().requires_grad_(True)
    h_ref = F_.silu(uu[:, :F]) * uu[:, F:]
    h_ref.backward(dh.double())
    h = ops.swiglu_fwd(u.to(DEV))
    du = ops.swiglu_bwd(u.to(DEV), dh.to(DEV))
    assert h.dtype == dtype and tuple(h.shape) == (rows, F) and tuple(du.shape) == (rows, 2 * F)
    tol = 1e-5 if dtype == torch.float32 else 3e-2
    assert (h.double().cpu() - h_ref.detach()).abs().max().item() <= tol * max(1.0, h_ref.abs().max().item())
    assert (du.double().cpu() - uu.grad).abs().max().item() <= tol * max(1.0, uu.grad.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swiglu_strided_rows_leave_the_pad_alone(ops, dtype):
    """gate | up rows with a pad behind them (ldu > 2F) and an output with a pad (ldh > F): same values, the pad keeps its bytes."""
    from eavqa_amd import _lib_llama
    rows, F, pad = 5, 32, 8
    buf = rnd(rows, 2 * F + pad, seed=3, dtype=dtype).to(DEV)
    out = torch.full((rows, F + pad), 7.0, dtype=dtype, device=DEV)
    _lib_llama.call("eavqa_swiglu_fwd", ops.dtype_id(dtype), rows, F, buf.data_ptr(), 2 * F + pad, out.data_ptr(), F + pad, ops._stream())
    want = ops.swiglu_fwd(buf[:, :2 * F].contiguous())
    assert torch.equal(out[:, :F], want) and bool((out[:, F:] == 7.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("F,ks", [(32, 1), (160, 4)])
def test_swiglu_splitk(ops, dtype, rows, F, ks):
    part = rnd(ks, rows, 2 * F, seed=1)
    u = part.double().sum(0)
    ref = F_.silu(u[:, :F]) * u[:, F:]
    h = ops.swiglu_splitk(part.to(DEV), dtype)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert (h.double().cpu() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


def test_bad_sizes_are_shape_errors_not_faults():
    from eavqa_amd import _lib, _lib_llama
    lib = _lib_llama.load()
    assert lib.eavqa_swiglu_fwd(1, 4, 6, 16, 12, 16, 6, None) == _lib.EAVQA_E_SHAPE
    assert lib.eavqa_swiglu_fwd(1, 4, 8, 16, 8, 16, 8, None) == _lib.EAVQA_E_SHAPE          # ldu < 2F
    assert lib.eavqa_swiglu_bwd(1, 4, 8, 16, 16, 16, 4, 16, 16, None) == _lib.EAVQA_E_SHAPE  # lddh < F
    assert lib.eavqa_swiglu_splitk(1, 4, 6, 16, 1, 16, 8, None) == _lib.EAVQA_E_SHAPE
    assert lib.eavqa_swiglu_splitk(7, 4, 8, 16, 1, 16, 8, None) == _lib.EAVQA_E_DTYPE
    assert lib.eavqa_swiglu_fwd(1, 0, 8, 16, 16, 16, 8, None) == _lib.EAVQA_E_ARG
