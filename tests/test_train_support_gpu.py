"""GPU: the small kernels around the training step's GEMMs - AdamW, cross-entropy, the greedy pick, LayerNorm / T5LayerNorm forward
and backward with the parameter gradients, column sums, the cast / copy kernels, the row plan, the scored-row selection and the
embedding assembly - at the sizes where their loops run more than once, their tails and strides matter and their branches differ.

References: the float64 restatements of tests/_train_ref.py (pinned to torch on the CPU by tests/test_train_ref_cpu.py), computed
from the operands as stored.  Tolerances are those of tests/test_ops_gpu.py: fp32 results within 1e-5 max(1, |ref|) of float64, bf16
results within 3e-2 (fp16 4e-3), integer / copy / cast kernels bit-exact; sums that combine through atomics get the worst-case bound
of an fp32 sum in any order, stated where used.  Output buffers start as NaN (-7 for integers) and are one row and a few columns
larger than needed: the surplus must come back untouched.

Which case enters which path (and the mutation that turns it red; "run" = built into a scratch copy of the library and run on the
MI355X, where exactly the cases named here failed; "read" = argued from the code):
  adamw_kernel, second grid stride          test_adamw_every_pass...[4195507-*], test_adamw_chunked...   `i2 = i + stride` -> `i` (run)
  adamw_kernel, tail / shadow kinds          test_adamw_every_pass...[1-*], [3-*], [1027-*]; bf16 / f32 / none     tail loop skipped (run)
  ce_fwd_kernel (V > 65 536)                test_cross_entropy_vocabulary_edges[65537], _extreme_rows[65537-65540]
                                            the -inf guard of its running maximum removed = the code before this file existed (run)
  ce_reduce_kernel, rows > 1024, `bad`      test_cross_entropy_more_rows...; ..._label_outside_the_vocabulary...  `r += 1024` -> leave (run)
  ce_fwd_row_kernel / ce_bwd_kernel edges   test_cross_entropy_vocabulary_edges, _extreme_rows[1025-1028]              (read)
  greedy_pick_kernel, V > 1024              test_greedy_pick_many_columns_per_thread       in-thread `>` -> `>=` (run)
  ln_bwd / ln_dparam: bf16 x, ragged, strides, lowp_out, alias, accumulate, one of two, row counts
                                            test_layernorm_backward_strided_ragged[*-bf16], test_layernorm_backward_variants
                                            ln_dparam_kernel leaves out one row in 16 (run); x read as fp32 when it is bf16 would
                                            read out of bounds: not run, any misread x moves dgamma by ~|dy|, far beyond the bound (read)
  ln_fwd / rms kernels, rows far from zero  test_norms_on_rows_far_from_zero       one-pass variance in ln_fwd_kernel (run)
  colsum atomics / cast_rows chunk stride / copy_rows 4-element path / guard_count `>`
                                            test_colsum[257.. 16500.. 300..], test_cast_rows[1-2100004], test_copy_rows...[*-12-bf16],
                                            test_guard_count      atomicAdd -> store, one pass only, path emptied, `>=` (run)
  row_plan_kernel: carry, waves, count loop test_row_plan_holes_chunks_and_many_samples    `carry` dropped (run: S > 64 cases red)
  select_rows_kernel chunk edges            test_select_rows_chunk_edges[1025], [2048]      `base += t` -> `base = t` (run)
  embed_assemble(_bwd), E > 1024            test_embed_assemble_wide_rows          second pass of `c += 1024` dropped (run)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _train_ref as R

DEV = "cuda"
NAN = float("nan")
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


rnd = R.rnd


def dev(t):
    return None if t is None else t.to(DEV)


def guarded(rows, cols, dtype, ld=None, c0=0, fill=NAN):
    """(buffer [rows + 1, ld] full of ``fill`` on the device, its [rows, cols] view at column ``c0``)."""
    ld = cols + 8 if ld is None else ld
    assert c0 + cols <= ld
    buf = torch.full((rows + 1, ld), fill, device=DEV, dtype=dtype)
    return buf, buf[:rows, c0:c0 + cols]


def surplus_untouched(buf, rows, cols, c0=0, fill=NAN):
    b = buf.cpu()
    outside = torch.ones(b.shape, dtype=torch.bool)
    outside[:rows, c0:c0 + cols] = False
    vals = b[outside]
    return bool(torch.isnan(vals).all()) if isinstance(fill, float) and math.isnan(fill) else bool((vals == fill).all())


def in_wider(t, ld, c0=4, poison=3e4):
    """``t`` [rows, cols] as a column slice (from column ``c0``) of a [rows, ld] device buffer whose other entries are large: a read
    outside the slice shows in every statistic."""
    rows, cols = t.shape
    buf = torch.full((rows, ld), poison, dtype=t.dtype)
    buf[:, c0:c0 + cols] = t
    return buf.to(DEV)[:, c0:c0 + cols]


def lds(cols, mode):
    """A leading dimension for a [rows, cols] slice at column 4 with ld = ``mode`` (0 or 4) mod 8: with 4, odd rows of a bf16 matrix
    start 8 bytes off a 16-byte boundary."""
    return (cols + 12 + 7) // 8 * 8 + mode


def within(got, ref, dtype=F32):
    """fp32 results: 1e-5 max(1, |ref|) elementwise; bf16: 3e-2; fp16: 4e-3 (header of tests/test_ops_gpu.py)."""
    got, ref = got.detach().cpu().double(), ref.double()
    if torch.isnan(got).any():
        return False
    err = (got - ref).abs()
    if dtype == F32:
        return bool((err <= 1e-5 * torch.clamp(ref.abs(), min=1.0)).all())
    return bool(err.max().item() <= (3e-2 if dtype == BF16 else 4e-3))


# =============================================================================================== a. AdamW
SHADOWS = {"bf16": BF16, "f32": F32, "none": None}


def run_adamw(ops, n, setting, shadow_dtype, bounds=None):
    """The 4 steps of a setting on the device, in one launch per step or one launch per slice ``bounds[i]:bounds[i+1]``."""
    step0, kw, _ = R.ADAMW_SETTINGS[setting]
    p, m, v, grads = R.adamw_inputs(n, setting)
    P, M, V = p.to(DEV), m.to(DEV), v.to(DEV)
    sh_buf = torch.full((n + 5,), NAN, device=DEV, dtype=shadow_dtype) if shadow_dtype is not None else None
    sh = sh_buf[:n] if sh_buf is not None else None
    bounds = [0, n] if bounds is None else bounds
    for i, g in enumerate(grads):
        G = g.to(DEV)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            ops.adamw(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], step0 + i, shadow=sh[lo:hi] if sh is not None else None, **kw)
    torch.cuda.synchronize()
    return P.cpu(), M.cpu(), V.cpu(), (sh_buf.cpu() if sh_buf is not None else None)


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("setting", list(R.ADAMW_SETTINGS))
@pytest.mark.parametrize("n", [R.ADAMW_BIG_N, 1, 3, 4, 1027])
def test_adamw_every_pass_of_the_grid_stride_loop(ops, n, setting, shadow):
    """n = 4 195 507: both float4 of a loop iteration (``two``), a third pass that only part of the grid takes, a 3-element tail;
    n < 4: the tail alone.  atol 2e-7 / rtol 1e-6 against the float64 formula (exact fp32 evaluation is within 1e-9 + rtol of it:
    test_train_ref_cpu.py); the shadow is the parameter rounded once.  The moments are held to the same atol; their rtol allows for the
    one thing the parameter is insensitive to: the kernel receives beta as a float, so its (1 - beta) differs from the reference's
    by up to 2^-24 / (1 - beta) relative (4.7e-5 for beta2 = 0.999), and so does every moment."""
    want_p, want_m, want_v = R.adamw_expected(n, setting)
    kw = R.ADAMW_SETTINGS[setting][1]
    P, M, V, sh = run_adamw(ops, n, setting, SHADOWS[shadow])
    for got, want, rtol in ((P, want_p, 1e-6), (M, want_m, 1e-6 + 2.0 ** -24 / (1 - kw["beta1"])), (V, want_v, 1e-6 + 2.0 ** -24 / (1 - kw["beta2"]))):
        assert not torch.isnan(got).any()
        assert bool(((got.double() - want).abs() <= 2e-7 + rtol * want.abs()).all()), ((got.double() - want).abs() - rtol * want.abs()).max().item()
    if sh is not None:
        assert torch.equal(sh[:n], P.to(SHADOWS[shadow])) and torch.isnan(sh[n:]).all()


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("setting", ["defaults", "late"])
def test_adamw_chunked_update_is_bit_equal_to_one_launch(ops, setting, shadow):
    """trainers/optim.py promises that updating a flat buffer slice by slice gives the bits of one launch.  Four slices whose bounds
    are multiples of 4 and none longer than 2 097 152 elements (each takes the single-pass path; the last ends at n and so owns the
    3-element tail) against the one-launch run, which walks the two-float4 loop three times."""
    n = R.ADAMW_BIG_N
    bounds = [0, 1_000_000, 2_097_152, 3_100_000, n]
    assert all(b % 4 == 0 for b in bounds[:-1]) and max(hi - lo for lo, hi in zip(bounds[:-1], bounds[1:])) <= 2_097_152
    one = run_adamw(ops, n, setting, SHADOWS[shadow])
    sliced = run_adamw(ops, n, setting, SHADOWS[shadow], bounds)
    for a, b in zip(one[:3], sliced[:3]):
        assert torch.equal(a, b)
    if one[3] is not None:
        assert torch.equal(one[3][:n], sliced[3][:n]) and torch.isnan(sliced[3][n:]).all()


# =============================================================================================== b. cross-entropy
def check_ce(ops, logits, labels, V, ldd, grads_atol=None, lowp=False):
    """ce_fwd + ce_bwd of one case against R.ce: exact count, loss and row_lse within 1e-5 max(1, |ref|), finite gradients that sum
    to zero per row and agree with the reference, zeros in the pad columns.

    Gradient bound: count * |d - ref| <= 2^-22 max(1, |lse|) + 1e-6 per element and for the row sum (summed in float64 here).  The
    kernel's lse is stored in fp32 after one fp32 addition (two half-ulps, 2^-23 |lse|, doubled for margin); exp(x - lse) inherits
    that as a relative error, and softmax - onehot is at most 1 in magnitude and sums to 0."""
    want_loss, want_count, want_lse, want_d = R.ce(logits, labels, V)
    lg, lb = logits.to(DEV), labels.to(DEV)
    loss, count, row_lse = ops.ce_fwd(lg, lb, V)
    assert count.item() == want_count
    if math.isnan(want_loss):
        assert math.isnan(loss.item())
    else:
        assert abs(loss.item() - want_loss) <= 1e-5 * max(1.0, abs(want_loss)), (loss.item(), want_loss)
    rl = R.row_labels_of(labels)
    scored = (rl >= 0) & (rl < V)
    lse = row_lse.cpu().double()
    assert bool(((lse - want_lse).abs() <= 1e-5 * torch.clamp(want_lse.abs(), min=1.0)).all()), (lse, want_lse)   # 0 where not scored
    gs = torch.ones(1, device=DEV)
    for dtype in (F32, BF16) if lowp else (F32,):
        d = ops.ce_bwd(lg, lb, V, row_lse, count, gs, dtype, ldd).cpu().double()
        assert d.shape[1] == ldd and torch.isfinite(d).all() and (d[:, V:] == 0).all()
        assert (d[~scored] == 0).all()
        if dtype == BF16:
            assert torch.allclose(d[:, :V], want_d, atol=1e-3, rtol=1e-2)   # as test_cross_entropy_forward_backward
            continue
        bound = (2.0 ** -22 * torch.clamp(want_lse.abs(), min=1.0) + 1e-6) / max(want_count, 1)
        assert bool((d[:, :V].sum(-1).abs() <= bound).all()), (d[:, :V].sum(-1), bound)
        assert bool(((d[:, :V] - want_d).abs() <= bound[:, None]).all()), (d[:, :V] - want_d).abs().max().item()
        if grads_atol is not None:
            assert (d[:, :V] - want_d).abs().max().item() <= grads_atol
    return loss, count


def test_cross_entropy_more_rows_than_reduce_threads(ops):
    """1500 rows: ce_reduce_kernel's 1024 threads each take a second row.  About a third of the labels ignored, one whole sample."""
    B, S, V, ld = 5, 300, 7, 8
    logits = torch.full((B * S, ld), 3e38)
    logits[:, :V] = rnd(B * S, V, seed=1, scale=3.0)
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[torch.rand(B, S, generator=g) < 0.25] = -100
    labels[3] = -100
    assert 0.25 < (labels == -100).float().mean().item() < 0.45
    check_ce(ops, logits, labels, V, ld, grads_atol=1e-7, lowp=True)


@pytest.mark.parametrize("V", [1, 1023, 1025, 65535, 65536, 65537])
def test_cross_entropy_vocabulary_edges(ops, V):
    """One column, one below / above the 1024 threads of the register-resident kernel, its last two sizes, and the first size of
    the online max / sum kernel; 3 scored rows and one ignored, pad columns that hold 3e38."""
    ld = (V + 3) // 4 * 4 + 4
    logits = torch.full((4, ld), 3e38)
    logits[:, :V] = rnd(4, V, seed=1, scale=3.0)
    labels = torch.tensor([V - 1, -100, 0, V // 2])
    check_ce(ops, logits, labels, V, ld)


@pytest.mark.parametrize("V,ld", [(1025, 1028), (65537, 65540)])
def test_cross_entropy_extreme_rows(ops, V, ld):
    """A row times 1000, a row that starts with 100 -inf entries, a row shifted by +5000, a 2e4 spike at the label (loss 0): through
    the register kernel (V = 1025) and the online kernel (V = 65 537), whose running maximum starts at -inf."""
    x, lab = R.ce_extreme_rows(V)
    logits = torch.full((6, ld), 3e38)
    logits[:, :V] = x
    check_ce(ops, logits, lab, V, ld)


@pytest.mark.parametrize("bad", ["V", "-5"])
@pytest.mark.parametrize("V", [7, 65537])
def test_cross_entropy_label_outside_the_vocabulary_poisons_the_loss(ops, V, bad):
    ld = (V + 3) // 4 * 4
    logits = torch.zeros(4, ld)
    logits[:, :V] = rnd(4, V, seed=1, scale=3.0)
    labels = torch.tensor([1, V if bad == "V" else -5, -100, V - 1])
    loss, count = check_ce(ops, logits, labels, V, ld)
    assert math.isnan(loss.item()) and count.item() == 2


def test_guard_count(ops):
    for count, capacity, start, poisoned in ((8, 8, 1.5, False), (9, 8, 1.5, True), (0, 0, 1.5, False), (3, 8, NAN, True)):
        loss = torch.tensor([start, -2.0], device=DEV)
        ops.guard_count(torch.tensor([count, 10 ** 6], dtype=torch.int32, device=DEV), capacity, loss)
        got = loss.cpu()
        assert math.isnan(got[0].item()) if poisoned else got[0].item() == start
        assert got[1].item() == -2.0


# =============================================================================================== c. greedy pick
def test_greedy_pick_many_columns_per_thread(ops):
    """V = 50 257 over 1024 threads: each thread sees ~49 columns and its own first maximum has to survive."""
    V, ld, B = 50257, 50264, 5
    logits = torch.full((B, ld), 3e38)
    logits[:, :V] = rnd(B, V, seed=1)
    logits[0, 17] = logits[0, 17 + 1024] = 50.0                  # same thread: the earlier column
    logits[1, 2000] = logits[1, 1999 + 1024 * 3] = 60.0          # different threads: the smaller index
    logits[2, V - 1] = 70.0
    logits[3, :V] = R.NEG_INF                                    # torch.argmax of an all -inf row is 0
    logits[4, 5] = 80.0
    want = logits[:, :V].argmax(-1).tolist()
    assert want == [17, 2000, V - 1, 0, 5]
    L = logits.to(DEV)
    raw = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
    toks = torch.full((B + 1, 6), -7, dtype=torch.int64, device=DEV)
    unf = torch.tensor([1, 1, 1, 1, 0, -7], dtype=torch.int32, device=DEV)
    alive = torch.zeros(3, dtype=torch.int32, device=DEV)
    lp = torch.full((B + 1,), NAN, device=DEV)
    ops.greedy_pick(L, V, 42, V - 1, raw[:B], toks[:B, 2], unf[:B], lp[:B], any_unfinished=alive[1:2])
    assert raw.cpu().tolist() == want + [-7]
    assert toks[:, 2].cpu().tolist() == [17, 2000, V - 1, 0, 42, -7]          # the finished row emits pad
    assert unf.cpu().tolist() == [1, 1, 0, 1, 0, -7]                          # row 2 just produced eos
    assert alive.cpu().tolist() == [0, 1, 0]
    assert (toks.cpu()[:, [0, 1, 3, 4, 5]] == -7).all()
    want_lp = torch.log_softmax(logits[:3, :V].double(), -1).max(-1).values
    assert (lp.cpu()[:3].double() - want_lp).abs().max().item() <= 1e-5 and math.isnan(lp.cpu()[B].item())
    ops.greedy_pick(L, V, 42, None, raw[:B], toks[:B, 3], unf[:B])             # eos None: raw tokens, flags untouched
    assert toks[:, 3].cpu().tolist() == want + [-7] and unf.cpu().tolist() == [1, 1, 0, 1, 0, -7]


# =============================================================================================== d. LayerNorm / T5LayerNorm
SHAPES = [(1, 4), (63, 68), (64, 260), (65, 1028), (257, 4092)]     # cols / 4 ragged inside every NV instantiation; rows around a block row
POISON = {F32: 1e30, BF16: 1e30, F16: 6e4}


def norm_inputs(rows, cols, dtype, mode):
    x = (rnd(rows, cols, seed=1) * 2 + 0.5).to(dtype)
    gamma, beta = rnd(cols, seed=2) * 0.2 + 1, rnd(cols, seed=3) * 0.1
    return x, in_wider(x, lds(cols, mode), poison=POISON[dtype]), gamma, beta


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("mode", [4, 0])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_layernorm_forward_strided_ragged(ops, rows, cols, mode, dtype):
    x, X, gamma, beta = norm_inputs(rows, cols, dtype, mode)
    want_y, want_mean, want_rstd = R.layernorm_fwd(x, gamma, beta, 1e-5)
    ld = lds(cols, 4 - mode)
    buf, y = guarded(rows, cols, dtype, ld, 4)
    _, mean, rstd = ops.layernorm_fwd(X, dev(gamma), dev(beta), 1e-5, dtype, save_stats=True, out=y)
    assert within(y, want_y, dtype) and surplus_untouched(buf, rows, cols, 4)
    assert (mean.cpu().double() - want_mean).abs().max().item() <= 1e-5
    assert ((rstd.cpu().double() - want_rstd).abs() / want_rstd).max().item() <= 1e-5


def dparam_ok(got, want, abs_sum, rows):
    """|got - want| <= (rows + 8) 2^-24 sum_r |term|: the worst case of an fp32 sum of ``rows`` terms in ANY order (blocks combine
    through atomics) plus four roundings per term.  A missing or doubled row is off by ~1 / rows of the sum of magnitudes, three
    orders of magnitude beyond this."""
    got = got.cpu().double()
    return bool(torch.isfinite(got).all()) and bool(((got - want).abs() <= (rows + 8) * 2.0 ** -24 * abs_sum).all())


def run_layernorm_bwd(ops, rows, cols, dtype, mode, *, gamma=True, alias=False, prefill=False, want_dgamma=True, want_dbeta=True, x=None):
    if x is None:
        x = (rnd(rows, cols, seed=1) * 2 + 0.5).to(dtype)
    g = rnd(cols, seed=2) * 0.2 + 1 if gamma else None
    dy, dres = rnd(rows, cols, seed=4, dtype=dtype), rnd(rows, cols, seed=5)
    _, mean64, rstd64 = R.layernorm_fwd(x, None, None, 1e-5)
    mean, rstd = mean64.float(), rstd64.float()                             # what the kernel reads and what the reference reads
    want_dx, want_dg, want_db, abs_g, abs_b = R.layernorm_bwd(x, dy, g, mean, rstd, dres)
    ld, ld2 = lds(cols, mode), lds(cols, 4 - mode)
    X, DY = in_wider(x, ld, poison=POISON[dtype]), in_wider(dy, ld2, poison=POISON[dtype])
    dx_buf, dx = guarded(rows, cols, F32, ld2, 4)
    if alias:
        dx.copy_(dres)                                                     # models/clipcap.py: dres IS the output buffer
        DRES = dx
    else:
        DRES = in_wider(dres, ld2, poison=1e30)
    lp_buf, lowp = guarded(rows, cols, dtype, ld, 4)
    init_g = rnd(cols, seed=6) if prefill else torch.zeros(cols)
    init_b = rnd(cols, seed=7) if prefill else torch.zeros(cols)
    dg_buf, db_buf = torch.full((cols + 8,), NAN, device=DEV), torch.full((cols + 8,), NAN, device=DEV)
    dg_buf[:cols], db_buf[:cols] = init_g.to(DEV), init_b.to(DEV)
    out = ops.layernorm_bwd(X, DY, dev(g), dev(mean), dev(rstd), dres=DRES, dgamma=dg_buf[:cols] if want_dgamma else None,
                            dbeta=db_buf[:cols] if want_dbeta else None, out=dx, lowp_out=lowp)
    assert out.data_ptr() == dx.data_ptr()
    assert within(dx, want_dx) and surplus_untouched(dx_buf, rows, cols, 4)
    assert within(lowp, want_dx, dtype) and surplus_untouched(lp_buf, rows, cols, 4)
    assert torch.isnan(dg_buf[cols:]).all() and torch.isnan(db_buf[cols:]).all()
    # a prefilled accumulator adds one rounding of |initial + gradient| <= |initial| + sum |term|
    if want_dgamma:
        assert dparam_ok(dg_buf[:cols], init_g.double() + want_dg, abs_g + init_g.abs().double(), rows)
    else:
        assert torch.equal(dg_buf[:cols].cpu(), init_g)
    if want_dbeta:
        assert dparam_ok(db_buf[:cols], init_b.double() + want_db, abs_b + init_b.abs().double(), rows)
    else:
        assert torch.equal(db_buf[:cols].cpu(), init_b)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [4, 0])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_layernorm_backward_strided_ragged(ops, rows, cols, mode, dtype):
    """bf16: x, dy and the second copy of dx are bf16 slices (the ``x_f32 == 0`` loads of ln_bwd_kernel and ln_dparam_kernel)."""
    run_layernorm_bwd(ops, rows, cols, dtype, mode)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("variant", ["no_gamma", "alias", "prefill", "only_dgamma", "only_dbeta"])
def test_layernorm_backward_variants(ops, variant, dtype):
    kw = dict(no_gamma=dict(gamma=False), alias=dict(alias=True), prefill=dict(prefill=True), only_dgamma=dict(want_dbeta=False, prefill=True),
              only_dbeta=dict(want_dgamma=False, prefill=True))[variant]
    run_layernorm_bwd(ops, 65, 1028, dtype, 4, **kw)


def test_layernorm_forward_without_gamma_and_beta(ops):
    rows, cols = 65, 1028
    for dtype in (F32, BF16):
        x, X, gamma, beta = norm_inputs(rows, cols, dtype, 4)
        for g, b in ((None, None), (gamma, None), (None, beta)):
            y = ops.layernorm_fwd(X, dev(g), dev(b), 1e-5, dtype)
            assert within(y, R.layernorm_fwd(x, g, b, 1e-5)[0], dtype)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("mode", [4, 0])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_rmsnorm_forward_backward_strided_ragged(ops, rows, cols, mode, dtype):
    """x in fp32 / bf16 / fp16 (the residual stream of T0 is fp16-storable); y and dy are fp32 for fp32 x and bf16 otherwise."""
    x, X, gamma, _ = norm_inputs(rows, cols, dtype, mode)
    lowp = F32 if dtype == F32 else BF16
    want_y, want_rstd = R.rmsnorm_fwd(x, gamma, 1e-6)
    y, rstd = ops.rmsnorm_fwd(X, dev(gamma), 1e-6, lowp, save_stats=True)
    assert within(y, want_y, lowp)
    assert ((rstd.cpu().double() - want_rstd).abs() / want_rstd).max().item() <= 1e-5
    assert within(ops.rmsnorm_fwd(X, None, 1e-6, lowp), R.rmsnorm_fwd(x, None, 1e-6)[0], lowp)
    dy, dres = rnd(rows, cols, seed=4, dtype=lowp), rnd(rows, cols, seed=5)
    rs = want_rstd.float()
    want_dx = R.rmsnorm_bwd(x, dy, gamma, rs, dres)
    ld2 = lds(cols, 4 - mode)
    dx_buf, dx = guarded(rows, cols, F32, ld2, 4)
    lp_buf, lp = guarded(rows, cols, lowp, lds(cols, mode), 4)
    ops.rmsnorm_bwd(X, in_wider(dy, ld2, poison=1e30), dev(gamma), dev(rs), dres=in_wider(dres, ld2, poison=1e30), out=dx, lowp_out=lp)
    assert within(dx, want_dx) and surplus_untouched(dx_buf, rows, cols, 4)
    assert within(lp, want_dx, lowp) and surplus_untouched(lp_buf, rows, cols, 4)
    dx.copy_(dres)                                                          # dres aliasing the output, no gamma
    ops.rmsnorm_bwd(X, in_wider(dy, ld2, poison=1e30), None, dev(rs), dres=dx, out=dx)
    assert within(dx, R.rmsnorm_bwd(x, dy, None, rs, dres))


@pytest.mark.parametrize("cols", R.OFFSET_COLS)
def test_norms_on_rows_far_from_zero(ops, cols):
    """x = 256 + k / 8: the variance (~0.4) is 2^-17 of E[x^2].  Every intermediate of a two-pass kernel up to the variance sum is
    exact on these rows (test_train_ref_cpu.py), so the ordinary fp32 tolerance holds; a one-pass E[x^2] - mean^2 is off by more than
    1e-3.  Runs every kernel that computes or consumes row statistics, the decode-path split-K finishers included."""
    rows = 6
    x = R.offset_rows(rows, cols)
    gamma, beta = rnd(cols, seed=2) * 0.2 + 1, rnd(cols, seed=3) * 0.1
    X, G, Bt = dev(x), dev(gamma), dev(beta)
    want_y, want_mean, want_rstd = R.layernorm_fwd(x, gamma, beta, 1e-5)
    y, mean, rstd = ops.layernorm_fwd(X, G, Bt, 1e-5, F32, save_stats=True)
    assert within(y, want_y)
    assert (mean.cpu().double() - want_mean).abs().max().item() <= 1e-5
    assert ((rstd.cpu().double() - want_rstd).abs() / want_rstd).max().item() <= 1e-5
    assert within(ops.layernorm_splitk(X, G, Bt, 1e-5, F32, part=None), want_y)
    run_layernorm_bwd(ops, rows, cols, F32, 0, x=x)
    want_r, want_rs = R.rmsnorm_fwd(x, gamma, 1e-6)
    yr, rs = ops.rmsnorm_fwd(X, G, 1e-6, F32, save_stats=True)
    assert within(yr, want_r) and ((rs.cpu().double() - want_rs).abs() / want_rs).max().item() <= 1e-5
    assert within(ops.rmsnorm_splitk(X, G, 1e-6, F32, part=None), want_r)
    dy, dres = rnd(rows, cols, seed=4), rnd(rows, cols, seed=5)
    dx = ops.rmsnorm_bwd(X, dev(dy), G, dev(want_rs.float()), dres=dev(dres))
    assert within(dx, R.rmsnorm_bwd(x, dy, gamma, want_rs.float(), dres))


# =============================================================================================== e. seq.hip
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,c0", [(1, 4, 0), (255, 70, 0), (257, 70, 0), (16500, 70, 0), (64, 1280, 0), (300, 72, 128)])
def test_colsum(ops, rows, cols, c0, dtype):
    """One block row without atomics (rows <= 256), atomics (257), the capped grid where a block strides over rows (16 500); the
    last case is a column slice [:, 128:] of a wider matrix (models/clipcap.py, the bias gradient of a fused projection).
    Bound: rows 2^-24 sum_r |x|, the worst case of an fp32 sum of ``rows`` terms in any order."""
    full = rnd(rows, c0 + cols, seed=1, dtype=dtype)
    x = full[:, c0:]
    X = full.to(DEV)[:, c0:]
    want, mag = x.double().sum(0), x.double().abs().sum(0)
    buf = torch.full((cols + 8,), NAN, device=DEV)
    ops.colsum(X, buf[:cols], accumulate=False)
    got = buf.cpu().double()
    assert torch.isnan(got[cols:]).all() and bool(((got[:cols] - want).abs() <= rows * 2.0 ** -24 * mag).all())
    init = rnd(cols, seed=2)
    buf[:cols] = init.to(DEV)
    ops.colsum(X, buf[:cols], accumulate=True)
    got = buf.cpu().double()
    bound = (rows + 1) * 2.0 ** -24 * (mag + init.abs().double())          # one more term: the initial contents
    assert torch.isnan(got[cols:]).all() and bool(((got[:cols] - (want + init.double())).abs() <= bound).all())


def cast_specials():
    """float32 bit patterns whose bf16 rounding is decided at the edge: ties to even both ways, +-0, +-inf, the largest finite (-> inf),
    subnormals (smallest, largest, one that rounds up to the smallest normal), roundings that carry into the exponent, NaN."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x00000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x3FFFFFFF, 0x3FFF8000,
            0xBFFFFFFF, 0x477FE000, 0x7FC00000, 0x7F800001]
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(F32)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,cols,ldx,ldy", [(1, 2_100_004, None, None), (3, 68, 72, 80), (2048, 4, None, None)])
def test_cast_rows(ops, rows, cols, ldx, ldy, dtype):
    """One row of millions of columns (the flat-parameter shadow: blockIdx.y strides over 1024-column chunks, the last chunk ragged),
    strided rows, many one-vector rows.  Bit-equal to torch's round-to-nearest-even cast; a NaN stays a NaN."""
    x = rnd(rows, cols, seed=1)
    sp = cast_specials()
    flat = x.view(-1)
    for start in (0, flat.numel() - sp.numel()):                            # the specials at both ends of the data
        flat[start:start + sp.numel()] = sp
    ldx, ldy = ldx or cols, ldy or cols + 4
    X = in_wider(x, ldx, c0=0, poison=1e30) if ldx != cols else x.to(DEV)
    buf, y = guarded(rows, cols, dtype, ldy, 0)
    out = ops.cast_rows(X, dtype, out=y)
    assert out.data_ptr() == y.data_ptr() and surplus_untouched(buf, rows, cols, 0)
    got, want = y.cpu(), x.to(dtype)
    nan = torch.isnan(want)
    assert nan.sum().item() == 4 and torch.equal(torch.isnan(got), nan)
    ints = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(got.contiguous().view(ints)[~nan], want.view(ints)[~nan])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cols", [8, 12, 2560])
@pytest.mark.parametrize("S", [1, 5])
def test_copy_rows_into_a_cache(ops, S, cols, dtype):
    """K rows out of a [B*S, 3*cols] QKV-like buffer into a NaN-filled [B*t_max, cols] cache at row ``dst_row0`` of every sample.
    cols = 12 in bf16 is no multiple of the 16-byte vector: the 4-element path."""
    B, t_max, row0 = 3, 9, 2
    qkv = rnd(B * S, 3 * cols, seed=1, dtype=dtype)
    src = qkv.to(DEV)[:, cols:2 * cols]
    buf, cache = guarded(B * t_max, cols, dtype, cols + 8, 0)
    ops.copy_rows(src, cache, B, S, cols, S, t_max, row0)
    want = torch.full((B, t_max, cols), NAN, dtype=dtype)
    want[:, row0:row0 + S] = qkv[:, cols:2 * cols].view(B, S, cols)
    got = cache.cpu().view(B, t_max, cols)
    ints = torch.int16 if dtype == BF16 else torch.int32
    moved = ~torch.isnan(want)
    assert torch.equal(torch.isnan(got), ~moved) and torch.equal(got.contiguous().view(ints)[moved], want.view(ints)[moved])
    assert surplus_untouched(buf, B * t_max, cols, 0)


PLAN_CASES = {"holes": (9, 150, dict()), "empty": (9, 150, dict(empty=4)), "full": (9, 150, dict(full=2)), "many": (300, 5, dict(empty=7, full=260)),
              "chunk": (4, 64, dict()), "chunk+1": (4, 65, dict())}


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("case", list(PLAN_CASES))
def test_row_plan_holes_chunks_and_many_samples(ops, case, pack, with_labels):
    """S > 64: the running offset crosses 64-position chunks; B > 4: a wave takes several samples; B > 256: the counting loop runs
    twice; masks with holes; samples that keep nothing or everything.  Exact against the loops of R.row_plan."""
    B, S, kw = PLAN_CASES[case]
    g = torch.Generator().manual_seed(11)
    mask = R.holey_mask(B, S, **kw)
    src = torch.randint(-40, 1000, (B, S), generator=g).int()
    pos = torch.randint(0, 2048, (B, S), generator=g).int()
    labels = torch.randint(0, 50, (B, S), generator=g) if with_labels else None
    want = R.row_plan(mask, labels, src, pos, pack)
    got = ops.build_row_plan(dev(mask), dev(labels), dev(src), dev(pos), pack)
    M = int(want[0][-1])
    assert M == (int(mask.sum()) if pack else B * S)
    assert torch.equal(got[0].cpu(), want[0])
    for a, b in zip(got[1:], want[1:]):
        assert torch.equal(a.cpu()[:M], b)


@pytest.mark.parametrize("M", [1, 1024, 1025, 2048])
def test_select_rows_chunk_edges(ops, M):
    labels = torch.where(torch.rand(M, generator=torch.Generator().manual_seed(M)) < 0.6, torch.arange(M) % 500, torch.full((M,), -100))
    labels[M - 1] = 7                                                       # the last row of the last chunk is scored
    want_idx, want_lab, want_n = R.select_rows(labels, M)
    idx, lab, cnt = ops.select_rows(dev(labels), want_n + 3)
    assert cnt.item() == want_n and torch.equal(idx.cpu()[:want_n], want_idx) and torch.equal(lab.cpu()[:want_n], want_lab)
    assert (idx.cpu()[want_n:] == 0).all() and (lab.cpu()[want_n:] == -100).all()
    half = want_n // 2
    idx, lab, cnt = ops.select_rows(dev(labels), half)                      # capacity below the count: the first ones, counted in full
    assert cnt.item() == want_n and torch.equal(idx.cpu(), want_idx[:half]) and torch.equal(lab.cpu(), want_lab[:half])
    idx, lab, cnt = ops.select_rows(dev(labels), 0)
    assert cnt.item() == want_n and idx.numel() == 0 and lab.numel() == 0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_embed_assemble_wide_rows(ops, dtype):
    """E = 1284 > 1024: a thread's second pass over the row, with a ragged end; dx is a column slice."""
    g = torch.Generator().manual_seed(1)
    B, L, T, E, V = 3, 4, 9, 1284, 100
    wte, wpe = rnd(V, E, dtype=dtype, seed=1), rnd(32, E, dtype=dtype, seed=2)
    prefix = rnd(B * L, E, dtype=dtype, seed=3)
    tok = torch.randint(0, V, (B, T), generator=g)
    src, msk, pos = ops.build_prefix_rows(dev(tok), torch.ones(B, T, dtype=torch.long, device=DEV), L, 0)
    rows = B * (L + T)
    buf, out = guarded(rows, E, F32, E + 8, 4)
    x = ops.embed_assemble(src, pos, dev(wte), dev(prefix), dev(wpe), out=out)
    ref = torch.cat([prefix.view(B, L, E).float(), wte.float()[tok]], dim=1) + wpe.float()[: L + T][None]
    assert torch.equal(x.cpu().view(B, L + T, E), ref) and surplus_untouched(buf, rows, E, 4)
    x0 = ops.embed_assemble(src, None, dev(wte), dev(prefix), None)         # no position table (OPT adds it elsewhere)
    assert torch.equal(x0.cpu().view(B, L + T, E), torch.cat([prefix.view(B, L, E).float(), wte.float()[tok]], dim=1))
    dx = rnd(rows, E, seed=4)
    dp = ops.embed_assemble_bwd(src, in_wider(dx, E + 12, poison=1e30), B * L, dtype)
    assert torch.equal(dp.float().cpu().view(B, L, E), dx.view(B, L + T, E)[:, :L].to(dtype).float())
