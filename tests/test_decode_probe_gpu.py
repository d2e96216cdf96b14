"""GPU: the decode step's GEMM and reduction kernels (csrc/decode.hip, csrc/decode_direct.hip) on the exact probes of tests/_gemm_probe.py.

Split-K: every slice of the partial sums must EQUAL the float64 product of its own k-range (not only their sum), for every variant of
eavqa_gemm_splitk_ex and for eavqa_gemm_fp8_splitk, on strided operands with NaN pads.  The finish passes: 1 / 2 / 3 destination segments
with their own row strides and guards, slice counts on either side of the eight the kernels keep in flight, every activation.  The
LayerNorm / RMSNorm passes over partial sums: every width of the row (NV = 1, 2, 4, 8 float4 per thread), row strides larger than the
row, x_out bit for bit on integers.  eavqa_gemm_decode: strided operands, T5's gate with a bias, ragged segments and statistics,
norm-on-load under every forced fragment count.
"""
import math

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


def to_dev(bufs):
    return {nm: P.on_device(b, vw, DEV) for nm, (b, vw) in bufs.win.items()}


def back(bufs, dev, names):
    got = P.Bufs()
    for nm in names:
        vw = bufs.win[nm][1]
        b = dev[nm][0].cpu()
        got.win[nm] = (b, b.as_strided(tuple(vw.shape), vw.stride(), vw.storage_offset()))
    return got


def collect(cases, run):
    failed = []
    for c in cases:
        try:
            run(c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("sel", sorted({c.sel for c in P.SPLITK_CASES if not c.fp8}))
def test_splitk_every_slice_is_its_own_k_range(ops, sel):
    from eavqa_amd import _lib

    def run(c):
        ks, KS = c.resolve(_lib.load().eavqa_gemm_splitk_plan)
        bufs, v = P.materialize_splitk(c, ks, KS)
        ref = P.reference_splitk(c, ks, KS, bufs, v)
        dev = to_dev(bufs)
        ops.gemm_splitk(dev["a"][1], dev["b"][1], ks=ks, unroll=c.sel, out=dev["part"][1])
        P.check_splitk(c, ks, ref, back(bufs, dev, ["part"]))
    collect([c for c in P.SPLITK_CASES if not c.fp8 and c.sel == sel], run)


def test_fp8_splitk_every_slice_is_its_own_k_range(ops):
    """Integer e4m3 values, power-of-two scales: the block-scaled 16x16x128 instruction with unit block scales is exact on them."""
    from eavqa_amd import _lib

    def run(c):
        ks, KS = c.resolve(_lib.load().eavqa_gemm_fp8_splitk_plan)
        bufs, v = P.materialize_splitk(c, ks, KS)
        ref = P.reference_splitk(c, ks, KS, bufs, v)
        dev = to_dev(bufs)
        ops.gemm_fp8_splitk(dev["a"][1], bufs.a_scale.to(DEV), dev["b"][1], bufs.b_scale, ks=ks, out=dev["part"][1])
        P.check_splitk(c, ks, ref, back(bufs, dev, ["part"]))
    collect([c for c in P.SPLITK_CASES if c.fp8], run)


# ----------------------------------------------------------------------------------------------------------------------- finish
@pytest.mark.parametrize("n_seg", [1, 2, 3])
def test_splitk_finish_segments_slices_activations(ops, n_seg):
    def run(c):
        bufs, v = P.materialize_finish(c)
        ref = P.reference_finish(c, v)
        dev = to_dev(bufs)
        outs = [dev[f"out{j}"][1] for j in range(c.n_seg)]
        ops.splitk_finish(dev["part"][1].view(c.ks, c.M, c.N), outs, bias=dev["bias"][1][0] if c.bias else None, act=c.act,
                          residual=dev["res"][1] if c.ldr else None)
        P.check_finish(c, ref, back(bufs, dev, [f"out{j}" for j in range(c.n_seg)]))
    collect([c for c in P.FINISH_CASES if not c.gated and c.n_seg == n_seg], run)
    print("worst error / bound so far:", {k: round(x, 4) for k, x in sorted(P.WORST.items())})


def test_splitk_finish_gated(ops):
    from eavqa_amd import _lib

    def run(c):
        bufs, v = P.materialize_finish(c)
        ref = P.reference_finish(c, v)
        dev = to_dev(bufs)
        h = dev["out0"][1]
        _lib.call("eavqa_splitk_finish_gated", ops.dtype_id(h.dtype), c.M, c.N, dev["part"][1].data_ptr(), c.ks, _lib.ACT[c.act], h.data_ptr(),
                  h.stride(0), ops._stream())
        P.check_finish(c, ref, back(bufs, dev, ["out0"]))
    collect([c for c in P.FINISH_CASES if c.gated], run)
    print("worst error / bound so far:", {k: round(x, 4) for k, x in sorted(P.WORST.items())})


# --------------------------------------------------------------------------------------------------- norms over partial sums
def norm_rows(cols, ks):
    """Two row counts, because a slice of the partial sums is rows x cols: the decode maximum of 64 wherever the data stays small (narrow
    rows at every slice count, wide rows at ks = 9), else 3."""
    return 64 if (cols <= 2052 or ks == 9) else 3


def norm_inputs(cols, ks, seed):
    g = torch.Generator().manual_seed(seed)
    ROWS = norm_rows(cols, ks)
    x = P.ints(g, (ROWS, cols), -8, 8)
    x[:, 0] += 3.0                                        # (cols = 4: no constant rows)
    part = P.ints(g, (max(ks, 1), ROWS, cols), -2, 2)
    bias = P.ints(g, (cols,), -3, 3)
    gamma = 1.0 + 0.2 * torch.randn(cols, generator=g)
    beta = 0.1 * torch.randn(cols, generator=g)
    return x, part, bias, gamma, beta


def norm_call(ops, kind, out_dtype, cols, ks, x, part, bias, gamma, beta, eps, with_x_out=True):
    """One call of eavqa_layernorm_splitk / eavqa_rmsnorm_splitk / eavqa_layernorm_splitk_fp8 on windows: x_in, x_out, y with row strides
    larger than the row and one guard row each.  Returns (x_out window, y window, scales) as CPU (backing, view) pairs."""
    from eavqa_amd import _lib
    ROWS = x.shape[0]
    xb, xv = P.window(ROWS, cols, cols + 4, torch.float32, fill=P.NAN)
    xv.copy_(x)
    pb, pv = P.window(max(ks, 1) * ROWS, cols, cols, torch.float32, fill=P.NAN)
    pv.copy_(part.view(-1, cols))
    bb, bv = P.window(1, cols, cols, torch.float32, fill=P.NAN)
    bv.copy_(bias)
    ob, ov = P.window(ROWS, cols, cols + 8, torch.float32, fill=P.SENTINEL)
    ydt = torch.uint8 if kind == "fp8" else out_dtype
    yb, yv = P.window(ROWS, cols, cols + 12, ydt, fill=0x5A if kind == "fp8" else P.SENTINEL)
    d = {nm: P.on_device(b, vw, DEV) for nm, (b, vw) in dict(x=(xb, xv), p=(pb, pv), b=(bb, bv), o=(ob, ov), y=(yb, yv)).items()}
    gm, bt = gamma.float().to(DEV), beta.float().to(DEV)
    xo_ptr, xo_ld = (d["o"][1].data_ptr(), cols + 8) if with_x_out else (None, 0)
    p_ptr = d["p"][1].data_ptr() if ks else None
    sc = None
    if kind == "layer":
        _lib.call("eavqa_layernorm_splitk", ops.dtype_id(out_dtype), ROWS, cols, d["x"][1].data_ptr(), cols + 4, p_ptr, ks,
                  d["b"][1].data_ptr() if ks else None, xo_ptr, xo_ld, gm.data_ptr(), bt.data_ptr(), eps, d["y"][1].data_ptr(), cols + 12, ops._stream())
    elif kind == "rms":
        _lib.call("eavqa_rmsnorm_splitk", ops.dtype_id(out_dtype), ROWS, cols, d["x"][1].data_ptr(), cols + 4, p_ptr, ks, xo_ptr, xo_ld,
                  gm.data_ptr(), eps, d["y"][1].data_ptr(), cols + 12, ops._stream())
    else:
        sc = torch.empty(ROWS, device=DEV, dtype=torch.float32)
        _lib.call("eavqa_layernorm_splitk_fp8", ROWS, cols, d["x"][1].data_ptr(), cols + 4, p_ptr, ks, d["b"][1].data_ptr() if ks else None,
                  xo_ptr, xo_ld, gm.data_ptr(), bt.data_ptr(), eps, d["y"][1].data_ptr(), cols + 12, sc.data_ptr(), ops._stream())
        sc = sc.cpu()
    o_cpu, y_cpu = d["o"][0].cpu(), d["y"][0].cpu()
    return ((o_cpu, o_cpu.as_strided((ROWS, cols), (cols + 8, 1), 0)), (y_cpu, y_cpu.as_strided((ROWS, cols), (cols + 12, 1), 0)), sc)


@pytest.mark.parametrize("cols", P.LN_COLS)
@pytest.mark.parametrize("kind", ["layer", "rms"])
def test_norm_over_partial_sums(ops, kind, cols):
    """x_out = x_in + bias + the slices, bit for bit (integers); y against float64 at the bounds of test_layernorm_splitk /
    test_rmsnorm_splitk_adds_the_partial_sums_first; nothing written outside the windows; x_out = NULL writes the same y.  3 and 64 rows (norm_rows)."""
    failed = []
    for i, ks in enumerate(P.LN_KS):
        out_dtype = (torch.float32, torch.bfloat16)[(i + cols // 4) % 2]
        eps = 1e-5 if kind == "layer" else 1e-6
        x, part, bias, gamma, beta = norm_inputs(cols, ks, 100 * cols + ks)
        xs = x + ((part.sum(0) + (bias if kind == "layer" else 0.0)) if ks else 0.0)
        if kind == "layer":
            want = torch.nn.functional.layer_norm(xs, (cols,), gamma.double(), beta.double(), eps)
        else:
            want = xs * torch.rsqrt((xs ** 2).mean(-1, keepdim=True) + eps) * gamma.double()
        (ob, ov), (yb, yv), _ = norm_call(ops, kind, out_dtype, cols, ks, x, part, bias, gamma, beta, eps)
        tol = (2e-5 if out_dtype == torch.float32 else 2e-2) * max(1.0, want.abs().max().item())
        err = (yv.double() - want).abs().max().item()
        tag = f"{kind} cols={cols} ks={ks} {out_dtype}"
        if not torch.equal(ov.double(), xs):
            failed.append(f"{tag}: x_out is not x_in + bias + the slices: {P._first_diff(ov.double(), xs)}")
        if not (P.untouched(ob, ov) and P.untouched(yb, yv)):
            failed.append(f"{tag}: written outside the x_out / y windows")
        if not err <= tol:
            failed.append(f"{tag}: |y - reference| = {err:.3e} > {tol:.3e}")
        _, (yb2, yv2), _ = norm_call(ops, kind, out_dtype, cols, ks, x, part, bias, gamma, beta, eps, with_x_out=False)      # the same call without x_out
        as_bits = torch.int32 if out_dtype == torch.float32 else torch.int16
        if not torch.equal(yb2.view(as_bits), yb.view(as_bits)):
            failed.append(f"{tag}: y differs when x_out is NULL")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("cols", P.LN_COLS)
def test_layernorm_splitk_fp8_is_the_two_kernel_pair(ops, cols):
    """Byte for byte eavqa_layernorm_splitk (bf16) + eavqa_quantize_rows_fp8, on strided windows; the same x_out."""
    failed = []
    for ks in P.LN_KS:
        x, part, bias, gamma, beta = norm_inputs(cols, ks, 100 * cols + ks)
        (ob, ov), (yb, yv), _ = norm_call(ops, "layer", torch.bfloat16, cols, ks, x, part, bias, gamma, beta, 1e-5)
        q_ref, s_ref = ops.quantize_rows_fp8(yv.contiguous().to(DEV))
        (ob2, ov2), (qb, qv), sc = norm_call(ops, "fp8", None, cols, ks, x, part, bias, gamma, beta, 1e-5)
        if not (torch.equal(ob.view(torch.int32), ob2.view(torch.int32)) and torch.equal(sc, s_ref.cpu()) and torch.equal(qv, q_ref.cpu())):
            failed.append(f"cols={cols} ks={ks}: bytes / scales / x_out differ from the two-kernel pair")
        if not P.untouched(qb, qv, fill=0x5A):
            failed.append(f"cols={cols} ks={ks}: bytes written outside the window")
    assert not failed, "\n".join(failed)


def test_norm_over_partial_sums_rejects_wider_rows(ops):
    from eavqa_amd import _lib
    cols = P.LN_COLS_REJECTED
    x = torch.zeros(1, cols, device=DEV)
    g = torch.ones(cols, device=DEV)
    with pytest.raises(_lib.EavqaError, match="shape"):
        ops.layernorm_splitk(x, g, g, 1e-5, torch.float32)
    with pytest.raises(_lib.EavqaError, match="shape"):
        ops.rmsnorm_splitk(x, g, 1e-6, torch.float32)
    with pytest.raises(_lib.EavqaError, match="shape"):
        ops.layernorm_splitk_fp8(x, g, g, 1e-5)


# ---------------------------------------------------------------------------------------------------------- direct decode GEMM
def combine(stats, N, cols):
    """(mean, biased variance) of every row from the [M, n, 2] partials, in float64 (tests/test_decode_direct_gpu.py)."""
    s = stats.double().cpu()
    n_i = torch.tensor([min(cols, N - i * cols) for i in range(s.shape[1])], dtype=torch.float64)
    mean = s[:, :, 0].sum(1) / N
    m2 = (s[:, :, 1] + n_i * (s[:, :, 0] / n_i - mean[:, None]) ** 2).sum(1)
    return mean, m2 / N


def test_gemm_decode_exact(ops):
    """Strided A, B and residual with NaN pads, the gate with a bias, segments that no workgroup's columns divide, rotate: bit for bit;
    the statistics partials (the last one ragged) through what their consumer derives from them, at test_decode_direct_gpu.py's bounds -
    the sums themselves are integers and exact."""
    def run(c):
        bufs, v = P.materialize_decode(c)
        ref = P.reference_decode(c, v)
        dev = to_dev(bufs)
        names = [f"out{j}" for j in range(c.n_seg)]
        stats = ops.gemm_decode(dev["a"][1], dev["b"][1], [dev[n][1] for n in names], gated=c.gated, bias=dev["bias"][1][0] if c.bias else None,
                                act=c.act, residual=dev["res"][1] if c.residual else None, want_stats=c.want_stats, sel=c.sel)
        P.check_decode(c, ref, back(bufs, dev, names))
        if c.want_stats:
            cols = 16 * (c.sel & 0xF)
            n = (c.N + cols - 1) // cols
            assert stats.shape == (c.M, n, 2)
            sums = torch.stack([ref[:, i * cols:(i + 1) * cols].sum(1) for i in range(n)], 1)
            assert torch.equal(stats[:, :, 0].double().cpu(), sums), f"{c.name}: the partial sums of the statistics"
            mean, var = combine(stats, c.N, cols)
            want = ref.var(1, unbiased=False)
            assert (mean - ref.mean(1)).abs().max().item() <= 1e-4 * math.sqrt(c.K), c.name
            assert ((var - want).abs() / want).max().item() <= 1e-3, c.name
    collect(P.DECODE_CASES, run)


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


@pytest.mark.parametrize("norm", ["layer", "rms"])
@pytest.mark.parametrize("M,sel", [(9, 1), (16, 2), (7, 3), (16, 4), (32, 1), (17, 2), (32, 3), (64, 3), (9, 0x82), (33, 0x81)])
def test_gemm_decode_norm_on_load(ops, norm, M, sel):
    """The chain of test_norm_on_load_from_the_producers_statistics under every fragment count dd_pick instantiates for the fp32 stream
    (16 rows x 4 fragments included) and under rotate: the stream x1 is a strided window with NaN pads, the producer's statistics
    partials cover a column count (48) that does not divide K, the consumer's weights are strided.  Same reference, same bound."""
    E, F, cols_in = 320, 200, 48
    ctx, wo = rnd(M, E, seed=1, dtype=torch.bfloat16), rnd(E, E, seed=2, scale=0.03, dtype=torch.bfloat16)
    x, bo = rnd(M, E, seed=3) + 0.3, rnd(E, seed=4, scale=0.1)
    w1, b1 = rnd(F, E, seed=5, scale=0.03, dtype=torch.bfloat16), rnd(F, seed=6, scale=0.1)
    gamma, beta = 1.0 + rnd(E, seed=7, scale=0.2), rnd(E, seed=8, scale=0.1)
    xb, xv = P.on_device(*P.window(M, E, E + 4, torch.float32, fill=P.NAN), DEV)
    st = ops.gemm_decode(ctx.to(DEV), wo.to(DEV), [xv], bias=bo.to(DEV), residual=x.to(DEV), want_stats=True,
                         sel=3 if M <= 32 else 0x203)     # 48 columns a workgroup (above 32 rows: as two row groups - 64 rows x 3 fragments is no kernel)
    assert E % cols_in and st.shape == (M, (E + cols_in - 1) // cols_in, 2)
    wb, wv = P.window(F, E, E + 16, torch.bfloat16, fill=P.NAN)
    wv.copy_(w1)
    wb, wv = P.on_device(wb, wv, DEV)
    fb, fv = P.on_device(*P.window(M, F, F + 8, torch.bfloat16, fill=P.SENTINEL), DEV)
    ops.gemm_decode(xv, wv, [fv], norm=norm, gamma=gamma.to(DEV), beta=beta.to(DEV) if norm == "layer" else None, eps=1e-5, stats_in=st,
                    stats_in_cols=cols_in, bias=b1.to(DEV), act="relu", sel=sel)
    x1c = xv.cpu().double()
    if norm == "layer":
        a = torch.nn.functional.layer_norm(x1c, (E,), gamma.double(), beta.double(), 1e-5)
    else:
        a = x1c * torch.rsqrt((x1c ** 2).mean(-1, keepdim=True) + 1e-5) * gamma.double()
    a = a.float().to(torch.bfloat16)
    ref = torch.relu(a.double() @ w1.double().T + b1.double())
    f_cpu = fb.cpu()
    f_view = f_cpu.as_strided((M, F), (F + 8, 1), 0)
    assert P.untouched(f_cpu, f_view)
    err = (f_view.double() - ref).abs().max().item()
    assert err <= 2 ** -7 * max(1.0, ref.abs().max().item()) + 2e-4 * math.sqrt(E), err
