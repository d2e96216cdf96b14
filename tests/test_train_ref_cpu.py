"""CPU: the training-support reference (tests/_train_ref.py) is torch's - every restatement against float64 autograd or
``torch.optim.AdamW`` at 1e-12 relative - and the inputs the GPU tests use are usable: exact float32 arithmetic of the same formulas
stays inside the tolerances those tests assert, by the reference and an fp32 emulation alone."""
import math

import pytest
import torch

import _train_ref as R

F64 = torch.float64


def close(a, b, rel=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return bool(((a - b).abs() <= rel * torch.maximum(b.abs(), torch.ones_like(b))).all())


# ------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("setting", list(R.ADAMW_SETTINGS))
def test_adamw_step_is_torch_adamw(setting):
    n = 257
    step0, kw, _ = R.ADAMW_SETTINGS[setting]
    p, m, v, grads = R.adamw_inputs(n, setting)
    ref = p.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=kw["lr"], betas=(kw["beta1"], kw["beta2"]), eps=kw["eps"], weight_decay=kw["weight_decay"])
    opt.state[ref] = dict(step=torch.tensor(float(step0 - 1)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
    for g in grads:
        ref.grad = g.double() * kw["grad_scale"]
        opt.step()
    got_p, got_m, got_v = R.adamw_run(n, setting)
    assert close(got_p, ref.detach()) and close(got_m, opt.state[ref]["exp_avg"]) and close(got_v, opt.state[ref]["exp_avg_sq"])


@pytest.mark.parametrize("n", [200003, R.ADAMW_BIG_N])
@pytest.mark.parametrize("setting", list(R.ADAMW_SETTINGS))
def test_adamw_fp32_arithmetic_stays_inside_the_gpu_tolerance(setting, n):
    """atol 2e-7 / rtol 1e-6 (tests/test_ops_gpu.py::test_adamw_matches_torch) hold for exact fp32 evaluation after the 4 steps of
    every setting, at n = 200 003 and on the inputs of the GPU test itself (n = 4 195 507): worst excess over the rtol part 9.9e-10."""
    want, _, _ = R.adamw_expected(n, setting)
    got, _, _ = R.adamw_run(n, setting, R.adamw_step_fp32)
    excess = ((got.double() - want).abs() - 1e-6 * want.abs()).max().item()
    print(f"adamw fp32 emulation {setting} n={n}: worst excess over rtol {excess:.3g}")
    assert excess <= 2e-7


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("affine", [True, False])
def test_layernorm_is_torch_autograd(affine):
    rows, cols = 7, 36
    x = R.rnd(rows, cols, seed=1, dtype=F64) * 2 + 0.5
    g = (R.rnd(cols, seed=2, dtype=F64) * 0.2 + 1) if affine else None
    b = R.rnd(cols, seed=3, dtype=F64) * 0.1 if affine else None
    dy, dres = R.rnd(rows, cols, seed=4, dtype=F64), R.rnd(rows, cols, seed=5, dtype=F64)
    xx = x.clone().requires_grad_(True)
    gg = g.clone().requires_grad_(True) if affine else None
    bb = b.clone().requires_grad_(True) if affine else None
    y_ref = torch.nn.functional.layer_norm(xx, (cols,), gg, bb, 1e-5)
    y_ref.backward(dy)
    y, mean, rstd = R.layernorm_fwd(x, g, b, 1e-5)
    assert close(y, y_ref.detach()) and close(mean, x.mean(-1)) and close(rstd, 1 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5))
    dx, dgamma, dbeta, abs_g, abs_b = R.layernorm_bwd(x, dy, g, mean, rstd, dres)
    assert close(dx, dres + xx.grad)
    assert close(R.layernorm_bwd(x, dy, g, mean, rstd, None)[0], xx.grad)
    if affine:
        assert close(dgamma, gg.grad) and close(dbeta, bb.grad)
    assert (abs_g >= dgamma.abs()).all() and (abs_b >= dbeta.abs()).all() and close(abs_b, dy.abs().sum(0))


@pytest.mark.parametrize("affine", [True, False])
def test_rmsnorm_is_torch_autograd(affine):
    rows, cols = 7, 36
    x = R.rnd(rows, cols, seed=1, dtype=F64) * 2 + 0.5
    g = (R.rnd(cols, seed=2, dtype=F64) * 0.2 + 1) if affine else None
    dy, dres = R.rnd(rows, cols, seed=4, dtype=F64), R.rnd(rows, cols, seed=5, dtype=F64)
    xx = x.clone().requires_grad_(True)
    y_ref = xx * torch.rsqrt((xx * xx).mean(-1, keepdim=True) + 1e-6)      # HF modeling_t5.py:50-72
    if affine:
        y_ref = g * y_ref
    y_ref.backward(dy)
    y, rstd = R.rmsnorm_fwd(x, g, 1e-6)
    assert close(y, y_ref.detach())
    assert close(R.rmsnorm_bwd(x, dy, g, rstd, dres), dres + xx.grad) and close(R.rmsnorm_bwd(x, dy, g, rstd, None), xx.grad)


def test_references_widen_low_precision_inputs_without_rounding():
    x = R.rnd(3, 8, seed=1, dtype=torch.bfloat16)
    y, mean, _ = R.layernorm_fwd(x, None, None, 1e-5)
    assert y.dtype == F64 and close(mean, x.double().mean(-1))
    assert R.rmsnorm_fwd(x.to(torch.float16), None, 1e-6)[0].dtype == F64


@pytest.mark.parametrize("cols", R.OFFSET_COLS)
def test_offset_rows_need_two_passes_and_two_passes_suffice_in_fp32(cols):
    """Two-pass fp32 LayerNorm of the offset rows: within 1e-5 of float64.  One-pass E[x^2] - mean^2 in fp32: off by more than 1e-3
    (the variance, ~0.4, drowns in the rounding of E[x^2] ~ 65 536; measured 7.5e-3 / 1.3e-2 / 3.8e-2 at 256 / 1024 / 4096 columns)."""
    x = R.offset_rows(5, cols)
    want, mean, rstd = R.layernorm_fwd(x, None, None, 1e-5)
    mu = x.sum(-1, keepdim=True) / cols
    assert torch.equal(mu[:, 0].double(), mean)                            # exact, as the builder promises
    var = ((x - mu) ** 2).sum(-1, keepdim=True) / cols
    two = (x - mu) * torch.rsqrt(var + 1e-5)
    assert two.dtype == torch.float32 and (two.double() - want).abs().max().item() <= 1e-5
    one = torch.zeros_like(x)
    for r in range(x.shape[0]):                                             # sequential fp32 accumulation, as one thread would
        s = q = torch.tensor(0.0)
        for c in range(0, cols, 64):
            s = s + x[r, c:c + 64].sum()
            q = q + (x[r, c:c + 64] * x[r, c:c + 64]).sum()
        m1 = s / cols
        v1 = q / cols - m1 * m1
        one[r] = (x[r] - m1) * torch.rsqrt(torch.clamp(v1, min=0.0) + 1e-5)
    err = (one.double() - want).abs().max().item()
    print(f"one-pass fp32 LayerNorm on offset rows, cols={cols}: max error {err:.3g}")
    assert err > 1e-3


# ------------------------------------------------------------------------------------------------ cross-entropy
def _torch_ce(logits, row_labels, V):
    lg = logits[:, :V].double().clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lg, row_labels, ignore_index=-100)
    loss.backward()
    return loss.item(), lg.grad


def test_ce_is_torch_cross_entropy_with_shift_and_ignore():
    B, S, V, ld = 3, 6, 11, 12
    logits = R.rnd(B * S, ld, seed=1, scale=3.0, dtype=F64)
    labels = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(2))
    labels[0, :3] = -100
    labels[2] = -100
    rl = R.row_labels_of(labels)
    assert rl.view(B, S)[:, -1].eq(-100).all() and torch.equal(rl.view(B, S)[:, :-1], labels[:, 1:])
    want_loss, want_d = _torch_ce(logits, rl, V)
    loss, count, lse, d = R.ce(logits, labels, V)
    assert count == int((rl >= 0).sum()) and close(loss, want_loss) and close(d, want_d)
    keep = rl >= 0
    assert close(lse[keep], torch.logsumexp(logits[:, :V], -1)[keep]) and (lse[~keep] == 0).all()
    loss1, count1, _, d1 = R.ce(logits, rl, V)                             # one label per row: no shift
    assert count1 == count and loss1 == loss and torch.equal(d1, d)


def test_ce_label_rule():
    V = 5
    logits = R.rnd(4, 8, seed=1)
    for bad in (V, -5):
        loss, count, lse, d = R.ce(logits, torch.tensor([1, bad, -100, 4]), V)
        assert math.isnan(loss) and count == 2 and (d[1] == 0).all() and (d[2] == 0).all() and lse[1] == 0
        assert close(d[[0, 3]], _torch_ce(logits, torch.tensor([1, -100, -100, 4]), V)[1][[0, 3]])
    loss, count, _, d = R.ce(logits, torch.full((4,), -100), V)
    assert math.isnan(loss) and count == 0 and (d == 0).all()


@pytest.mark.parametrize("V", [1025, 65537])
def test_extreme_logit_rows_are_usable_in_fp32(V):
    """fp32 torch.cross_entropy on the extreme rows stays within 1e-5 max(1, |ref|) of float64 (measured 8.9e-8): the tolerance the
    GPU test asserts on these rows is the format's, not a favour to the kernel."""
    x, lab = R.ce_extreme_rows(V)
    loss, count, lse, d = R.ce(x, lab, V)
    assert count == 6 and math.isfinite(loss) and torch.isfinite(lse).all() and torch.isfinite(d).all()
    row = torch.nn.functional.cross_entropy(x, lab, reduction="none").double()
    want = lse - x.double()[torch.arange(6), lab]
    rel = ((row - want).abs() / torch.clamp(want.abs(), min=1.0)).max().item()
    print(f"fp32 cross_entropy on the extreme rows, V={V}: {rel:.3g}")
    assert rel <= 1e-5
    assert abs(want[3].item()) <= 1e-12 and (d.sum(-1).abs() <= 1e-12).all()


# ------------------------------------------------------------------------------------------------ row plan / scored rows
@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("with_labels", [True, False])
def test_row_plan_is_nonzero_indexing(pack, with_labels):
    B, S = 6, 70
    g = torch.Generator().manual_seed(7)
    mask = R.holey_mask(B, S, empty=1, full=4)
    src = torch.randint(-50, 100, (B, S), generator=g).int()
    pos = torch.randint(0, S, (B, S), generator=g).int()
    labels = torch.randint(0, 50, (B, S), generator=g) if with_labels else None
    cu, src_r, pos_r, lab_r, flat = R.row_plan(mask, labels, src, pos, pack)
    keep = mask.bool() if pack else torch.ones(B, S, dtype=torch.bool)
    want_flat = torch.nonzero(keep.flatten()).flatten()
    assert torch.equal(flat.long(), want_flat)
    assert cu.tolist() == [0] + keep.sum(1).cumsum(0).tolist()
    assert not pack or (cu[2] == cu[1] and cu[5] - cu[4] == S)             # the empty and the full sample
    assert torch.equal(src_r, src.flatten()[want_flat]) and torch.equal(pos_r, pos.flatten()[want_flat])
    shifted = torch.nn.functional.pad(labels, (0, 1), value=-100)[:, 1:] if with_labels else torch.full((B, S), -100)
    assert torch.equal(lab_r, shifted.flatten()[want_flat])


def test_select_rows_is_nonzero_indexing():
    lab = torch.tensor([-100, 3, 0, -100, -1, 7, 9])
    idx, sel, count = R.select_rows(lab, 10)
    want = torch.nonzero(lab >= 0).flatten()
    assert torch.equal(idx.long(), want) and torch.equal(sel, lab[want]) and count == 4
    idx, sel, count = R.select_rows(lab, 2)
    assert idx.tolist() == [1, 2] and sel.tolist() == [3, 0] and count == 4
    assert R.select_rows(lab, 0)[0].numel() == 0 and R.select_rows(lab, 0)[2] == 4
