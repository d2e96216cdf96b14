"""GPU: every tiled GEMM kernel and eavqa_gemm_fp8 on the exact probes of tests/_gemm_probe.py.

Each case runs ONE call on windows into flat buffers - operands with a row stride larger than their shape and NaN in every pad and guard
row, outputs surrounded by a sentinel - on small integers, so the result must EQUAL the float64 reference (`torch.equal`): strided
operands, guard columns and a guard row around C and aux_out, each of the epilogue's vector flags 0 on its own and all together (float32,
bf16 and half outputs and residuals, aux_out and aux_in), out and residual in one unaligned window, the LM head's `out = buf[:, :N]`.
The kernel is forced through ops.KernelSelect.gemm; tests/test_gemm_probe_cpu.py pins, without a GPU, that every case reaches the
kernel it names and that `check` rejects the address bugs these cases exist for.  The non-linear activations keep a bit-exact aux_out
and the bounds of tests/test_ops_gpu.py on the activated output.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _gemm_probe as P

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


def run_case(ops, c: P.GemmCase):
    bufs, v = P.materialize(c)
    ref = P.reference(c, bufs, v)
    dev = {nm: P.on_device(b, vw, DEV) for nm, (b, vw) in bufs.win.items()}
    kw = dict(act=c.act, alpha=c.alpha, out=dev["c"][1])
    if c.bias is not None:
        kw["bias"] = dev["bias"][1][0]
    if c.aux:
        kw["aux_in" if c.aux == "in" else "aux_out"] = dev["aux"][1]
    if c.res:
        kw["residual"] = dev["c"][1] if c.res == "inplace" else dev["res"][1]
    if c.dtype == "fp8":
        ops.gemm_fp8(dev["a"][1], bufs.a_scale.to(DEV), dev["b"][1], bufs.b_scale, tile=c.fp8_tile, **kw)
    else:
        if c.prefetch:
            kw["prefetch"] = torch.zeros(1 << 16, device=DEV, dtype=torch.bfloat16)
        ops.KernelSelect.gemm = c.knobs
        try:
            ops.gemm(dev["a"][1], dev["b"][1], a_kc=c.a_kc, b_kc=c.b_kc, **kw)
        finally:
            ops.KernelSelect.gemm = 0
    got = P.Bufs(win={nm: (b.cpu(), None) for nm, (b, _) in dev.items() if nm in ("c", "aux")})
    for nm in got.win:
        vw = bufs.win[nm][1]
        b = got.win[nm][0]
        got.win[nm] = (b, b.as_strided(tuple(vw.shape), vw.stride(), vw.storage_offset()))
    P.check(c, ref, got)


EXACT_TILES = sorted({c.tile for c in P.GEMM_CASES})


@pytest.mark.parametrize("tile", EXACT_TILES)
def test_exact_probes(ops, tile):
    """Every exact case of one kernel: strided, guarded, each alignment flag, in place, head layout (the aspects are in the case names)."""
    failed = []
    cases = [c for c in P.GEMM_CASES if c.tile == tile and c.act in P.EXACT_ACTS]
    assert cases
    for c in cases:
        try:
            run_case(ops, c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("tile", sorted({c.tile for c in P.GEMM_CASES if c.act in P.NONLINEAR}))
def test_nonlinear_activations_on_an_exact_preactivation(ops, tile):
    """tanh, gelu_new, quick_gelu, forward (float32 and storage-type output) and backward at aux_in: aux_out bit for bit, the activated
    output inside tol() of test_gemm_epilogue_forward / test_gemm_epilogue_activation_backward.  Worst error / bound over all kernels,
    measured on an MI355X: float32 operands 0.22 (forward, tanh) and 0.22 (backward, gelu_new); bf16 operands 0.09 with a bf16 output
    (its rounding), below 1e-3 with a float32 one."""
    failed = []
    for c in (c for c in P.GEMM_CASES if c.tile == tile and c.act in P.NONLINEAR):
        try:
            run_case(ops, c)
        except AssertionError as e:
            failed.append(str(e))
    print("worst error / bound so far:", {k: round(x, 4) for k, x in sorted(P.WORST.items())})
    assert not failed, "\n".join(failed)
