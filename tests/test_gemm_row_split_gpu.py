"""GPU: the row split of the 256 x 256 kernel on an eavqa_gemm_ln call.

A problem whose ragged last tile row costs a whole round of workgroups runs as two launches (csrc/gemm.hip: gemm(), rows_from()): the
256 x 256 kernel on the full tile rows and the last M % 256 rows as a call of their own, with every row-indexed pointer advanced - those
of the eavqa_gemm_ln block included (copy_out, stats_out, ln_stats, mean_out, rstd_out).  Checked as producer, as consumer and as both
against a float32 computation of the same operands and against the same call kept in one launch (selector bit 25), at the tolerances of
tests/test_gemm_ln_gpu.py.

The shape: N = 1024 and the smallest M up to 16 448 that eavqa_gemm_route sends to the 256 x 256 kernel with a row split as an eavqa_gemm_ln
call without knobs.  At K = 128 there is none (the full-line tiles are cheaper at every such M), at K = 1024 the first is M = 16 385 with one
ragged row; the test takes K = 1024 and the CLIP tower's M = 16 448 (64 ragged rows), and asserts that this is such a shape."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
M, N, K = 16448, 1024, 1024
BIG = 5
NO_ROW_SPLIT = 1 << 25


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


@pytest.fixture(scope="module")
def split(ops):
    from eavqa_amd import _lib
    rows = C.c_int(0)
    r = _lib.load().eavqa_gemm_route(1, 1, 1, M, N, K, 1, 0, C.byref(rows))
    assert r == BIG * 256 and 0 < rows.value == M % 256, "not a row-split problem of the 256 x 256 kernel any more: pick another shape"
    assert _lib.load().eavqa_gemm_route(1, 1, 1, M, N, K, 1, NO_ROW_SPLIT, C.byref(rows)) >= 0 and rows.value == 0
    return M % 256


@pytest.fixture(scope="module")
def problem():
    """Operands, the statistics of the rows of x in three unequal slots, and the float32 references (computed once, never written again)."""
    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale)
    x = (rnd(M, K) * 1.7 + 0.4).to(torch.bfloat16).to(DEV)
    w = rnd(N, K, scale=0.05).to(torch.bfloat16).to(DEV)
    bias, res = rnd(N, scale=0.1).to(DEV), (rnd(M, N) + 0.25).to(DEV)
    xf, wf = x.float(), w.float()
    cut = [0, K // 3, K // 2, K]
    st = torch.stack([torch.stack((xf[:, a:b].double().sum(1), (xf[:, a:b].double() ** 2).sum(1)), 1) for a, b in zip(cut, cut[1:])], 1).float().contiguous()
    c = wf.sum(1)
    mean = xf.double().mean(1)
    rstd = 1.0 / torch.sqrt(xf.double().var(1, unbiased=False) + 1e-5)
    acc = xf @ wf.T                                                                 # float32, exact operands
    plain = acc + bias + res
    folded = rstd.float()[:, None] * (acc - mean.float()[:, None] * c) + bias + res
    return dict(x=x, w=w, bias=bias, res=res, st=st, c=c, mean=mean, rstd=rstd, plain=plain, folded=folded)


def run(ops, p, mode, knobs):
    slots = (N + 63) // 64
    o = dict(out=torch.empty((M, N), device=DEV, dtype=torch.float32))
    kw = {}
    if mode in ("producer", "both"):
        o["copy"] = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        o["stats"] = torch.full((M, slots + 2, 2), float("nan"), device=DEV, dtype=torch.float32)
        kw.update(copy_out=o["copy"], stats_out=o["stats"])
    if mode in ("consumer", "both"):
        o["mean"] = torch.full((M,), float("nan"), device=DEV)
        o["rstd"] = torch.full((M,), float("nan"), device=DEV)
        kw.update(ln_stats=p["st"], ln_c=p["c"], ln_eps=1e-5, ln_save=(o["mean"], o["rstd"]))
    ops.KernelSelect.gemm = knobs
    try:
        ops.gemm(p["x"], p["w"], bias=p["bias"], residual=p["res"], out=o["out"], **kw)
    finally:
        ops.KernelSelect.gemm = 0
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("mode", ["producer", "consumer", "both"])
def test_row_split_with_the_ln_arguments(ops, split, problem, mode):
    p = problem
    got, one = run(ops, p, mode, 0), run(ops, p, mode, NO_ROW_SPLIT)
    consumer = mode != "producer"
    ref = p["folded"] if consumer else p["plain"]
    tol = (2 ** -8 * ref.abs().max().item() + 1e-3) if consumer else 2e-4 * math.sqrt(K)
    tail = slice(M - split, M)
    for name, o in (("split", got), ("one launch", one)):
        err = (o["out"] - ref).abs()
        print(f"{mode} {name}: max error {err.max().item():.3g} (last {split} rows {err[tail].max().item():.3g}), bound {tol:.3g}")
        assert err.max().item() <= tol
        if mode in ("producer", "both"):
            assert torch.equal(o["copy"], o["out"].to(torch.bfloat16))              # the copy is the stored value rounded once - of every row
            st, g64 = o["stats"].double(), o["out"].double()
            assert not torch.isnan(st).any()
            s, ss = st[:, :, 0].sum(1), st[:, :, 1].sum(1)
            assert (s - g64.sum(1)).abs().max().item() <= 1e-5 * g64.abs().sum(1).max().item()
            assert ((ss - (g64 ** 2).sum(1)).abs() / (g64 ** 2).sum(1)).max().item() <= 1e-5
            assert (st[:, (N + 63) // 64:] == 0).all()
        if consumer:
            assert not torch.isnan(o["mean"][tail]).any() and not torch.isnan(o["rstd"][tail]).any()      # the second launch wrote its rows
            assert (o["mean"].double() - p["mean"]).abs().max().item() <= 1e-5
            assert ((o["rstd"].double() - p["rstd"]).abs() / p["rstd"]).max().item() <= 1e-4
    assert (got["out"] - one["out"]).abs().max().item() <= tol
    if consumer:
        assert (got["mean"] - one["mean"]).abs().max().item() <= 1e-5
        assert ((got["rstd"] - one["rstd"]).abs() / one["rstd"]).max().item() <= 1e-4
