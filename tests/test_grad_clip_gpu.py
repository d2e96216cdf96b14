"""GPU: gradient-norm clipping with the non-finite guard - ``eavqa_grad_sumsq``, ``eavqa_clip_plan``, ``eavqa_adamw_clipped`` through
``ops``, ``FusedAdamW(max_grad_norm=...)`` and the executor's ``train.additional.gradient_clipping``.

References: tests/_clip_ref.py (float64; pinned to ``clip_grad_norm_`` + ``torch.optim.AdamW`` by tests/test_grad_clip_ref_cpu.py) and,
wherever the clip coefficient is 1, ``ops.adamw`` itself, bit for bit.  Tolerances: the norm within 2 float32 ulps of the float64 value
(the double sum is far below half an ulp, the square root and the cast cost at most one each); a workgroup's partial sum within 1e-11 of
the float64 sum of its slice (<= 8204 double additions of exact squares); updated parameters and moments within the tolerances of
tests/test_train_support_gpu.py::test_adamw_every_pass_of_the_grid_stride_loop (atol 2e-7, rtol 1e-6, the moments' rtol widened by the
float32 betas) - the clip coefficient is a float32 quotient, 2e-7 relative, inside what that rtol leaves.

grad_sumsq_kernel gives workgroup b the float4 [b * per, (b + 1) * per) of the gradient, per = ceil(n4 / P), n4 = n // 4,
P = min(2048, ceil(n4 / 2048)); a thread walks its slice in trips of four 16-byte loads, 1024 float4 per workgroup and trip; workgroup 0
adds the n % 4 tail.  Which size reaches which branch:
  n = 1, 3              n4 = 0: the tail alone, the load loop never entered
  n = 1027              n4 = 256: first load of the first trip for every thread, the other three masked; 3-element tail
  n = 8192              exactly one workgroup's slice (2048 float4): two full trips for every thread, no tail
  n = 8193              the same slice and a 1-element tail
  n = 8196              one float4 more: P = 2, per = 1025 - the second workgroup's slice is one float4 shorter than the first's
  n = 24599             P = 4, per = 1538: a partial second trip; the guard tests' size (the last workgroup owns float4 4614..6148)
  n = 16 797 219        n4 = 2048 * 2048 + 5000 > the cap: P = 2048, per = 2051 - a third trip that only 3 threads take, a short last
                        slice (907 float4), a 3-element tail
Mutations run on the MI355X (built into the library, this file run once): the fourth load of a trip dropped in grad_sumsq_kernel -> every
sumsq case from n = 8192 up red except [8192-mixed] and [8193-mixed] (the 1e18 element hides the rest there; "plain" does not), the clipped
update at n = 4 195 507 and both fit() cases red; the skip test removed from adamw_clipped_kernel -> every guard case red.
Input kinds: "plain" N(0, 1), every element matters (the partial sums catch one dropped element); "mixed" one element of 1e18 among
elements of 1e-18 and N(0, 1); "tiny" / "huge" everything scaled by 1e-18 / 1e18, whose squares leave float32's range on either side.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _clip_ref as C
import _train_ref as R

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
BF16, F32 = torch.bfloat16, torch.float32
SHADOWS = {"bf16": BF16, "f32": F32, "none": None}
CAP_N = 4 * (2048 * 2048 + 5000) + 3
SUMSQ_SIZES = [1, 3, 1027, 8192, 8193, 8196, 24599, CAP_N]
GUARD_N = 24599


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


def f32(x):
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def adamw_inputs(n, setting):
    """R.adamw_inputs, built once per case (read-only: every use copies to the device or clones)."""
    return R.adamw_inputs(n, setting)


def expected_partials(n):
    n4 = n // 4
    return max(1, min(2048, -(-n4 // 2048)))


@functools.lru_cache(maxsize=None)
def base_gradient(n):
    return R.rnd(n, seed=77)


def gradient(n, kind):
    g = base_gradient(n).clone()
    if kind == "mixed":
        g[1::3] = 1e-18
        g[(2 * n) // 3] = 1e18
    elif kind == "tiny":
        g *= 1e-18
    elif kind == "huge":
        g *= 1e18
    return g


def new_state(applied=0):
    st = torch.zeros(8, device=DEV, dtype=torch.int32)
    st[4] = applied
    return st


def read_state(st):
    """(norm, scale_eff, inv_bc1, inv_sqrt_bc2, applied, skipped, skip) of a state block."""
    host = st.cpu()
    f = host.view(F32)
    return (f[0].item(), f[1].item(), f[2].item(), f[3].item(), int(host[4]), int(host[5]), int(host[6]))


@functools.lru_cache(maxsize=None)
def table(beta1, beta2):
    from eavqa_amd.trainers.optim import bias_correction_table
    return bias_correction_table(beta1, beta2).to(DEV)


def measure(ops, G, pre_scale, max_norm, st, betas=(0.9, 0.999)):
    """grad_sumsq + clip_plan over the whole gradient -> (partials, surplus of the partials buffer)."""
    P = ops.grad_sumsq_partials(G.numel())
    buf = torch.full((P + 3,), NAN, device=DEV, dtype=torch.float64)
    ops.grad_sumsq(G, buf[:P])
    ops.clip_plan(buf[:P], pre_scale, max_norm, table(*betas), st)
    return buf[:P], buf[P:]


# =============================================================================================== a. sum of squares
@pytest.mark.parametrize("kind", ["plain", "mixed", "tiny", "huge"])
@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_every_trip_slice_and_tail(ops, n, kind):
    g = gradient(n, kind)
    G = g.to(DEV)
    P = ops.grad_sumsq_partials(n)
    assert P == expected_partials(n)
    pre = 1.0 / 64 if kind == "plain" else 1.0
    st = new_state()
    partials, surplus = measure(ops, G, pre, INF, st)
    torch.cuda.synchronize()
    assert torch.isnan(surplus).all()
    # every workgroup's partial sum against the float64 sum of its slice
    sq = g.double() ** 2
    n4 = n // 4
    per = -(-n4 // P)
    want = torch.zeros(P, dtype=torch.float64)
    for b in range(P):
        want[b] = sq[4 * min(b * per, n4):4 * min((b + 1) * per, n4)].sum()
    want[0] += sq[4 * n4:].sum()
    got = partials.cpu()
    assert bool(((got - want).abs() <= 1e-11 * want).all()), ((got - want).abs() / want.clamp_min(1e-300)).max().item()
    # the norm within 2 float32 ulps of the float64 value
    ref = f32(pre) * math.sqrt(float(sq.sum()))
    norm, scale_eff, _, _, applied, skipped, skip = read_state(st)
    print(f"sumsq n={n} {kind}: norm {norm!r} ref {ref!r} ulps {abs(norm - ref) / float(np.spacing(np.float32(ref))):.3f}")
    assert math.isfinite(norm) and abs(norm - ref) <= 2 * float(np.spacing(np.float32(ref)))
    assert (applied, skipped, skip) == (1, 0, 0) and scale_eff == f32(pre)
    # a second run on the same buffer: the same bits
    st2 = new_state()
    again, _ = measure(ops, G, pre, INF, st2)
    torch.cuda.synchronize()
    assert torch.equal(again.cpu().view(torch.int64), got.view(torch.int64)) and torch.equal(st2.cpu(), st.cpu())


def test_clip_plan_coefficient_and_counters(ops):
    """coef = min(1, max_norm / (norm + 1e-6)) in float32; the counters and the table row follow the applied count, also past the
    table's end."""
    n = 1027
    g = gradient(n, "plain")
    G = g.to(DEV)
    norm64 = 0.5 * math.sqrt(float((g.double() ** 2).sum()))
    tab = table(0.9, 0.999)
    st = new_state(applied=5)
    for i, max_norm in enumerate([norm64 * 4, norm64 / 4, INF, 1e-3]):
        measure(ops, G, 0.5, max_norm, st)
        norm, scale_eff, c1, c2, applied, skipped, skip = read_state(st)
        want = 0.5 * min(1.0, max_norm / (norm64 + 1e-6))
        assert abs(scale_eff - want) <= 4e-7 * want and (scale_eff == 0.5) == (max_norm > norm64)
        assert (applied, skipped, skip) == (6 + i, 0, 0) and (c1, c2) == tuple(tab[5 + i].tolist())
    st = new_state(applied=10 ** 6)
    measure(ops, G, 0.5, 1.0, st)
    assert read_state(st)[2:5] == (1.0, 1.0, 10 ** 6 + 1)


# =============================================================================================== b. update
def run_reference_adamw(ops, n, setting, shadow_dtype, steps):
    """``steps`` steps of ops.adamw from the inputs of a setting -> device tensors (P, M, V, shadow buffer)."""
    step0, kw, _ = R.ADAMW_SETTINGS[setting]
    p, m, v, grads = adamw_inputs(n, setting)
    P, M, V = p.to(DEV), m.to(DEV), v.to(DEV)
    sh_buf = torch.full((n + 5,), NAN, device=DEV, dtype=shadow_dtype) if shadow_dtype is not None else None
    for i in range(steps):
        ops.adamw(P, grads[i].to(DEV), M, V, step0 + i, shadow=sh_buf[:n] if sh_buf is not None else None, **kw)
    return P, M, V, sh_buf


def run_clipped(ops, n, setting, shadow_dtype, steps, max_norm, bounds=None):
    """The same steps through grad_sumsq + clip_plan + adamw_clipped (one launch, or one per slice ``bounds[i]:bounds[i + 1]``)."""
    step0, kw, _ = R.ADAMW_SETTINGS[setting]
    kw = dict(kw)
    pre = kw.pop("grad_scale")
    p, m, v, grads = adamw_inputs(n, setting)
    P, M, V = p.to(DEV), m.to(DEV), v.to(DEV)
    sh_buf = torch.full((n + 5,), NAN, device=DEV, dtype=shadow_dtype) if shadow_dtype is not None else None
    st = new_state(applied=step0 - 1)
    bounds = [0, n] if bounds is None else bounds
    for i in range(steps):
        G = grads[i].to(DEV)
        measure(ops, G, pre, max_norm, st, betas=(kw["beta1"], kw["beta2"]))
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            ops.adamw_clipped(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], st, shadow=sh_buf[lo:hi] if sh_buf is not None else None, **kw)
    return P, M, V, sh_buf, st


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.cpu(), b.cpu()
    size = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.view(size), b.view(size))


@pytest.mark.parametrize("max_norm", ["inf", "above"])
@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("setting", list(R.ADAMW_SETTINGS))
@pytest.mark.parametrize("n", [R.ADAMW_BIG_N, 1, 3, 4, 1027])
def test_not_clipped_is_bit_equal_to_adamw(ops, n, setting, shadow, max_norm):
    """coef == 1 (max_norm = inf, or a max_norm above every step's norm): 3 steps leave the bits ``ops.adamw`` leaves with the same step
    numbers and grad_scale - the bias corrections come from the table, the scale from the state block, the arithmetic is one body.  The
    ``late`` setting starts at t = 1000 (rows 999.. of the table)."""
    step0, kw, _ = R.ADAMW_SETTINGS[setting]
    bound = INF if max_norm == "inf" else 2.0 * kw["grad_scale"] * max(float(g.double().norm()) for g in adamw_inputs(n, setting)[3]) + 1.0
    want = run_reference_adamw(ops, n, setting, SHADOWS[shadow], 3)
    got = run_clipped(ops, n, setting, SHADOWS[shadow], 3, bound)
    torch.cuda.synchronize()
    for a, b in zip(got[:4], want):
        assert same_bits(a, b)
    norm, scale_eff, _, _, applied, skipped, skip = read_state(got[4])
    assert (applied, skipped, skip) == (step0 + 2, 0, 0) and scale_eff == f32(kw["grad_scale"])


@functools.lru_cache(maxsize=None)
def clipped_expected(n, setting):
    """4 steps of tests/_clip_ref.py with max_norm = 0.3 x the first step's norm -> (p, m, v, max_norm, steps that clipped)."""
    step0, kw, _ = R.ADAMW_SETTINGS[setting]
    kw = dict(kw)
    pre = f32(kw.pop("grad_scale"))
    p, m, v, grads = adamw_inputs(n, setting)
    max_norm = 0.3 * C.grad_norm(grads[0], pre)
    state, clipped = C.State(applied=step0 - 1), 0
    for g in grads:
        p, m, v = C.clipped_adamw_step(p, g, m, v, state, pre, max_norm, **kw)
        clipped += C.clip_coef(state.norm, max_norm) < 1.0
    return p, m, v, max_norm, clipped


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("setting", list(R.ADAMW_SETTINGS))
@pytest.mark.parametrize("n", [R.ADAMW_BIG_N, 1, 3, 4, 1027])
def test_clipped_update_matches_the_reference(ops, n, setting, shadow):
    want_p, want_m, want_v, max_norm, clipped = clipped_expected(n, setting)
    assert clipped >= 1
    kw = R.ADAMW_SETTINGS[setting][1]
    P, M, V, sh, st = run_clipped(ops, n, setting, SHADOWS[shadow], R.ADAMW_STEPS, max_norm)
    torch.cuda.synchronize()
    P, M, V = P.cpu(), M.cpu(), V.cpu()
    for got, want, rtol in ((P, want_p, 1e-6), (M, want_m, 1e-6 + 2.0 ** -24 / (1 - kw["beta1"])), (V, want_v, 1e-6 + 2.0 ** -24 / (1 - kw["beta2"]))):
        assert not torch.isnan(got).any()
        excess = ((got.double() - want).abs() - rtol * want.abs()).max().item()
        print(f"clipped n={n} {setting} {shadow}: worst |err| - rtol |ref| = {excess:.3g} (atol 2e-7)")
        assert bool(((got.double() - want).abs() <= 2e-7 + rtol * want.abs()).all()), excess
    if sh is not None:
        sh = sh.cpu()
        assert torch.equal(sh[:n], P.to(SHADOWS[shadow])) and torch.isnan(sh[n:]).all()
    assert read_state(st)[4:] == (R.ADAMW_SETTINGS[setting][0] - 1 + R.ADAMW_STEPS, 0, 0)


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("setting", ["defaults", "late"])
def test_chunked_clipped_update_is_bit_equal_to_one_launch(ops, setting, shadow):
    """The norm over the WHOLE gradient once, then the update slice by slice with the one state block (FusedAdamW.step(chunks=...)):
    the bits of the one-launch update.  Slices as in test_adamw_chunked_update_is_bit_equal_to_one_launch."""
    n = R.ADAMW_BIG_N
    bounds = [0, 1_000_000, 2_097_152, 3_100_000, n]
    max_norm = clipped_expected(n, setting)[3]
    one = run_clipped(ops, n, setting, SHADOWS[shadow], R.ADAMW_STEPS, max_norm)
    sliced = run_clipped(ops, n, setting, SHADOWS[shadow], R.ADAMW_STEPS, max_norm, bounds)
    torch.cuda.synchronize()
    for a, b in zip(one[:4], sliced[:4]):
        assert same_bits(a, b)
    assert torch.equal(one[4].cpu(), sliced[4].cpu())


# =============================================================================================== c. guard
GUARD_SPOTS = {"first": 0, "last_of_body": 4 * (GUARD_N // 4) - 1, "tail": GUARD_N - 1, "last_workgroup": 4 * 5000}


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("bad", [NAN, INF])
@pytest.mark.parametrize("spot", list(GUARD_SPOTS))
def test_a_non_finite_gradient_skips_the_step_on_the_device(ops, spot, bad, shadow):
    """Two applied steps, a step whose gradient holds one NaN / +Inf (first element; last element of the float4 body; a tail element; an
    element of the last of the 4 workgroups' slices), one more finite step: the bad step changes no bit of param, m, v, shadow and
    advances only the skipped count; the run equals ``ops.adamw`` at t = 1, 2, 3 over the three finite gradients, bit for bit."""
    n, setting = GUARD_N, "defaults"
    assert ops.grad_sumsq_partials(n) == 4 and GUARD_SPOTS["last_workgroup"] >= 4 * 3 * 1538
    _, kw, _ = R.ADAMW_SETTINGS[setting]
    kw = dict(kw)
    pre = kw.pop("grad_scale")
    p, m, v, grads = adamw_inputs(n, setting)
    P, M, V = p.to(DEV), m.to(DEV), v.to(DEV)
    sd = SHADOWS[shadow]
    sh_buf = torch.full((n + 5,), NAN, device=DEV, dtype=sd) if sd is not None else None
    sh = sh_buf[:n] if sd is not None else None
    st = new_state()

    def step(g):
        G = g.to(DEV)
        measure(ops, G, pre, INF, st)
        ops.adamw_clipped(P, G, M, V, st, shadow=sh, **kw)

    step(grads[0])
    step(grads[1])
    before = [t.clone() if t is not None else None for t in (P, M, V, sh_buf)]
    poisoned = grads[2].clone()
    poisoned[GUARD_SPOTS[spot]] = bad
    step(poisoned)
    torch.cuda.synchronize()
    for a, b in zip((P, M, V, sh_buf), before):
        assert same_bits(a, b)
    norm, scale_eff, _, _, applied, skipped, skip = read_state(st)
    assert not math.isfinite(norm) and scale_eff == 0.0 and (applied, skipped, skip) == (2, 1, 1)
    step(grads[3])
    torch.cuda.synchronize()
    assert read_state(st)[4:] == (3, 1, 0)
    rP, rM, rV = p.to(DEV), m.to(DEV), v.to(DEV)
    r_buf = torch.full((n + 5,), NAN, device=DEV, dtype=sd) if sd is not None else None
    for t, g in enumerate((grads[0], grads[1], grads[3]), start=1):
        ops.adamw(rP, g.to(DEV), rM, rV, t, shadow=r_buf[:n] if sd is not None else None, grad_scale=pre, **kw)
    torch.cuda.synchronize()
    for a, b in zip((P, M, V, sh_buf), (rP, rM, rV, r_buf)):
        assert same_bits(a, b)


def test_a_tail_only_gradient_is_guarded_too(ops):
    P, M, V = torch.ones(3, device=DEV), torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    st = new_state()
    G = torch.tensor([1.0, -INF, 2.0], device=DEV)
    measure(ops, G, 1.0, 1.0, st)
    ops.adamw_clipped(P, G, M, V, st, 1e-3)
    torch.cuda.synchronize()
    assert P.tolist() == [1.0] * 3 and M.tolist() == [0.0] * 3 and V.tolist() == [0.0] * 3 and read_state(st)[4:] == (0, 1, 1)


# =============================================================================================== d. model level
def make_executor(mapping_type, clipping):
    from conftest import load_golden
    from test_executor_gpu import FakeTokenizer
    from test_model_gpu import build_model
    from eavqa_amd.trainers.clipcap_executor import ClipCapExecutor
    from eavqa_amd.utils.config_system import load_config
    z = load_golden(f"clipcap_gpt2_{mapping_type}.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "vqa2", "clip_cap_gpt2_large.jsonnet"),
                      opts=["train.lr=0.01", "data_loader.type=DataLoaderVQA2", "data_loader.additional.max_target_length=4"])
    cfg.train.additional.gradient_clipping = clipping
    model = build_model(z, "gpt2", mapping_type, torch.float32)
    V, D = int(z["cfg"][0]), int(z["cfg"][6])
    tok = FakeTokenizer(V, eos=V - 1, bos=V - 2)
    loader = type("Loader", (), {"tokenizer": tok, "decoder_tokenizer": tok})()
    return ClipCapExecutor(cfg, loader, model=model, dtype=torch.float32, device=DEV), tok, V, D


def batches_for(tok, V, D):
    from test_executor_gpu import vqa_batch
    out = [vqa_batch(V, D, tok.bos_token_id, tok.eos_token_id, 100 + i) for i in range(6)]
    for b in out:
        b["clip_embeddings"] = b["clip_embeddings"].reshape(-1, D)
    return out


def view_norm(ex, scale):
    """scale x the L2 norm over the NAMED parameters' gradient views (float64 on the host): what clip_grad_norm_ would see."""
    total = sum(float((p.grad.detach().cpu().double() ** 2).sum()) for _, p in ex.model.clip_project.named_parameters())
    return scale * math.sqrt(total)


@pytest.mark.parametrize("mapping_type", ["mlp", "transformer"])
def test_fit_clips_logs_the_norm_and_resumes_from_a_checkpoint(mapping_type):
    """3 optimiser steps of ``fit()`` with accumulate_grad_batches = 2 and ``gradient_clipping`` = half the first step's norm (taken from
    a ``fit()`` with clipping off).  Per step: the logged train/grad_norm equals the norm over the parameters' gradient views to rtol
    1e-5 (a kernel that wrote into the flat buffer's pad elements would show here, and the pads are checked to be zero); the flat
    parameters equal the replay of the same accumulated gradients through tests/_clip_ref.py within the update tolerances.  A
    checkpoint taken after step 2, loaded into a fresh executor, continues with the bits of the original's step 3."""
    ex0, tok, V, D = make_executor(mapping_type, 0)
    batches = batches_for(tok, V, D)
    ex0.fit(batches[:2], accumulate_grad_batches=2)
    assert "train/grad_norm" not in ex0.logged
    max_norm = 0.5 * view_norm(ex0, 0.5)

    ex, _, _, _ = make_executor(mapping_type, max_norm)
    fl = ex.model.clip_project.flat
    named = torch.zeros(fl.numel, dtype=torch.bool)
    for name, (off, shape) in fl.offsets.items():
        named[off:off + math.prod(shape)] = True
    assert not bool(named.all())                                   # the layout has pad elements
    p, m, v = fl.master.detach().cpu().double(), torch.zeros(fl.numel, dtype=torch.float64), torch.zeros(fl.numel, dtype=torch.float64)
    state, kw = C.State(), dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    ck = None
    for s in range(3):
        lr = ex.scheduler.get_last_lr()[0] if ex.scheduler else 0.01
        ex.fit(batches[2 * s:2 * s + 2], accumulate_grad_batches=2)
        assert ex.optimizer.max_grad_norm == max_norm
        logged = ex.logged["train/grad_norm"]
        assert logged.is_cuda and ex.logged["train/skipped_steps"].is_cuda
        want = view_norm(ex, 0.5)
        grad = fl.grad.detach().cpu()
        assert bool((grad[~named] == 0).all())
        assert abs(logged.item() - want) <= 1e-5 * want, (logged.item(), want)
        p, m, v = C.clipped_adamw_step(p, grad, m, v, state, 0.5, max_norm, lr=lr, **kw)
        assert C.clip_coef(state.norm, max_norm) < 1.0 or s > 0
        got = fl.master.detach().cpu().double()
        assert bool(((got - p).abs() <= 2e-7 + 1e-6 * p.abs()).all()), (s, (got - p).abs().max().item())
        assert bool(((ex.optimizer.m.cpu().double() - m).abs() <= 2e-7 + (1e-6 + 2.0 ** -24 / 0.1) * m.abs()).all())
        assert bool(((ex.optimizer.v.cpu().double() - v).abs() <= 2e-7 + (1e-6 + 2.0 ** -24 / 0.001) * v.abs()).all())
        assert int(ex.optimizer.applied_steps.item()) == s + 1 and int(ex.logged["train/skipped_steps"].item()) == 0
        if s == 1:
            ck = ex.state_dict()
            assert ck["optimizer"]["step"] == 2 and ck["optimizer"]["skipped_steps"] == 0
    ex2, _, _, _ = make_executor(mapping_type, max_norm)
    ex2.configure_optimizers()
    ex2.load_state_dict(ck)
    assert ex2.global_step == 2 and int(ex2.optimizer.applied_steps.item()) == 2
    ex2.fit(batches[4:6], accumulate_grad_batches=2)
    fl2 = ex2.model.clip_project.flat
    assert torch.equal(fl2.master, fl.master) and torch.equal(ex2.optimizer.m, ex.optimizer.m) and torch.equal(ex2.optimizer.v, ex.optimizer.v)
    assert ex2.logged["train/grad_norm"].item() == ex.logged["train/grad_norm"].item()


@pytest.mark.parametrize("clipping,calls", [(0, (3, 0, 0, 0)), (1e9, (0, 3, 3, 3))])
def test_with_the_key_at_zero_fit_launches_none_of_the_new_kernels(monkeypatch, clipping, calls):
    """``gradient_clipping: 0`` (every shipped config): 3 optimiser steps call ops.adamw 3 times and grad_sumsq / clip_plan / adamw_clipped
    never; with the key set the counts are the other way round (so the wrappers do count)."""
    from eavqa_amd import ops
    seen = {}
    for name in ("adamw", "grad_sumsq", "clip_plan", "adamw_clipped"):
        def wrapped(*a, _f=getattr(ops, name), _n=name, **k):
            seen[_n] = seen.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    ex, tok, V, D = make_executor("mlp", clipping)
    ex.fit(batches_for(tok, V, D), accumulate_grad_batches=2)
    assert ex.global_step == 3
    assert tuple(seen.get(k, 0) for k in ("adamw", "grad_sumsq", "clip_plan", "adamw_clipped")) == calls


def test_fused_adamw_chunked_step_with_clipping_is_bit_equal_to_one_launch():
    """``FusedAdamW(max_grad_norm=...).step(chunks=...)``: the two norm kernels first on the optimiser's stream, then the chunks - the
    bits of the one-launch step, and the accessors read the state block behind that stream."""
    from eavqa_amd.models.clipcap import FlatParams
    from eavqa_amd.trainers.optim import FusedAdamW
    shapes = [("a.weight", (300, 70)), ("a.bias", (300,)), ("b.weight", (70, 300)), ("b.bias", (70,))]
    finals = []
    for chunked in (False, True):
        fl = FlatParams(shapes, DEV, BF16)
        fl.master.copy_(R.rnd(fl.numel, seed=5).to(DEV))
        opt = FusedAdamW(fl, lr=1e-2, max_grad_norm=3.0)
        lo = fl.range_of("a.weight")[0]
        chunks = [(0, lo), (lo, fl.numel)]
        norms = []
        for s in range(3):
            fl.grad.copy_(R.rnd(fl.numel, seed=20 + s).to(DEV))
            opt.step(grad_scale=0.5, chunks=chunks if chunked else None)
            norms.append(opt.grad_norm.clone())
        fl.wait_ready()
        torch.cuda.synchronize()
        finals.append((fl.master.clone(), fl.shadow.clone(), opt.m.clone(), opt.v.clone(), [x.item() for x in norms], opt.state_dict()["step"]))
    for a, b in zip(finals[0][:4], finals[1][:4]):
        assert same_bits(a, b)
    assert finals[0][4] == finals[1][4] and finals[0][5] == finals[1][5] == 3
