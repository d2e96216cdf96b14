"""GPU: every index of the AdamW kernels' unrolled grid-stride loop (csrc/optim.hip: at most ADAMW_MAX_BLOCKS workgroups of ADAMW_THREADS
threads, ADAMW_UNROLL grid strides per loop trip).

One *iteration* is what the full capped grid covers per loop trip: 256 x 256 x 4 float4 = 1 048 576 floats.  The sizes are the smallest
at which each part of that loop can go wrong: 3 (tail only), 1 027 (a partial first stride + tail), one iteration - 4 (the last float4
of the fourth stride missing), exactly one iteration, one iteration + 4 (a second trip of one float4), two iterations + 7 (a third trip
and a 3-element tail).  ``ops.adamw`` and ``ops.adamw_clipped`` (coefficient 1 - max_norm = inf - with one skipped step in the middle:
a gradient holding an inf), each without a shadow and with a bf16 shadow.  Every case is checked two ways:

  * against the float64 references of tests/_train_ref.py / tests/_clip_ref.py at the tolerances of tests/test_train_support_gpu.py
    (atol 2e-7, rtol 1e-6; the moments' rtol widened by 2^-24 / (1 - beta), the kernel's float beta); the shadow is the parameter
    rounded once, the surplus of its buffer untouched;
  * bit for bit against the same entry point applied to consecutive slices of 262 144 floats (4-aligned; 65 536 float4 = one per thread of
    256 workgroups: no thread makes a second stride or a second trip), which pins every index of the unrolled loop without a tolerance.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _clip_ref as C
import _train_ref as R

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
ITERATION = 256 * 256 * 4 * 4          # floats per loop trip of the full grid: ADAMW_MAX_BLOCKS * ADAMW_THREADS * ADAMW_UNROLL float4
SLICE = 262_144
SIZES = [3, 1027, ITERATION - 4, ITERATION, ITERATION + 4, 2 * ITERATION + 7]
SHADOWS = {"none": None, "bf16": torch.bfloat16}
STEP0, KW, _ = R.ADAMW_SETTINGS["late"]          # t = 1000.., random moments: every term of the update is live
BAD_STEP = 1                                     # the clipped runs' second gradient holds an inf


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


@functools.lru_cache(maxsize=None)
def inputs(n, entry):
    """(p, m, v, gradients) on the CPU, read-only: 2 steps for adamw, 3 for clipped (the middle one non-finite)."""
    p, m, v, grads = R.adamw_inputs(n, "late")
    if entry == "adamw":
        return p, m, v, grads[:2]
    bad = grads[1].clone()
    bad[(2 * n) // 3] = INF
    return p, m, v, [grads[0], bad, grads[2]]


@functools.lru_cache(maxsize=None)
def expected(n, entry):
    p, m, v, grads = inputs(n, entry)
    if entry == "adamw":
        for i, g in enumerate(grads):
            p, m, v = R.adamw_step(p, g, m, v, STEP0 + i, **KW)
        return p, m, v
    kw = dict(KW)
    pre = float(torch.tensor(kw.pop("grad_scale"), dtype=torch.float32))
    state = C.State(applied=STEP0 - 1)
    for g in grads:
        p, m, v = C.clipped_adamw_step(p, g, m, v, state, pre, INF, **kw)
    assert (state.applied, state.skipped) == (STEP0 + 1, 1)
    return p, m, v


def run(ops, n, entry, shadow_dtype, sliced):
    """The steps of a case on the device, one launch per step or one per slice -> (P, M, V, shadow buffer) on the CPU."""
    from eavqa_amd.trainers.optim import bias_correction_table
    p, m, v, grads = inputs(n, entry)
    P, M, V = p.to(DEV), m.to(DEV), v.to(DEV)
    sh_buf = torch.full((n + 5,), NAN, device=DEV, dtype=shadow_dtype) if shadow_dtype is not None else None
    bounds = list(range(0, n, SLICE)) + [n] if sliced else [0, n]
    kw = dict(KW)
    if entry == "clipped":
        pre = kw.pop("grad_scale")
        st = torch.zeros(8, device=DEV, dtype=torch.int32)
        st[4] = STEP0 - 1
        table = bias_correction_table(kw["beta1"], kw["beta2"]).to(DEV)
        partials = torch.empty(ops.grad_sumsq_partials(n), device=DEV, dtype=torch.float64)
    for i, g in enumerate(grads):
        G = g.to(DEV)
        if entry == "clipped":                       # the norm over the WHOLE gradient once, then the update launch by launch
            ops.grad_sumsq(G, partials)
            ops.clip_plan(partials, pre, INF, table, st)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            sh = sh_buf[lo:hi] if sh_buf is not None else None
            if entry == "clipped":
                ops.adamw_clipped(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], st, shadow=sh, **kw)
            else:
                ops.adamw(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], STEP0 + i, shadow=sh, **kw)
    torch.cuda.synchronize()
    if entry == "clipped":
        assert st.cpu()[4:7].tolist() == [STEP0 + 1, 1, 0]          # two applied steps, one skipped, the last one not
    return P.cpu(), M.cpu(), V.cpu(), (sh_buf.cpu() if sh_buf is not None else None)


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("entry", ["adamw", "clipped"])
@pytest.mark.parametrize("n", SIZES)
def test_every_index_of_the_unrolled_loop(ops, n, entry, shadow):
    dtype = SHADOWS[shadow]
    P, M, V, sh = run(ops, n, entry, dtype, sliced=False)
    want_p, want_m, want_v = expected(n, entry)
    for name, got, want, rtol in (("p", P, want_p, 1e-6), ("m", M, want_m, 1e-6 + 2.0 ** -24 / (1 - KW["beta1"])),
                                  ("v", V, want_v, 1e-6 + 2.0 ** -24 / (1 - KW["beta2"]))):
        assert not torch.isnan(got).any()
        excess = ((got.double() - want).abs() - rtol * want.abs()).max().item()
        print(f"n={n} {entry} {shadow} {name}: worst |err| - rtol |ref| = {excess:.3g} (atol 2e-7)")
        assert excess <= 2e-7, (name, excess)
    if sh is not None:
        assert torch.equal(bits(sh[:n]), bits(P.to(dtype))) and torch.isnan(sh[n:]).all()
    sliced = run(ops, n, entry, dtype, sliced=True)
    for name, a, b in zip("pmv", (P, M, V), sliced):
        differ = int((bits(a) != bits(b)).sum())
        assert differ == 0, f"{name}: {differ} of {n} elements differ from the slice-by-slice run"
    if sh is not None:
        assert torch.equal(bits(sh[:n]), bits(sliced[3][:n])) and torch.isnan(sliced[3][n:]).all()


def test_the_skipped_step_alone_leaves_every_bit(ops):
    """The clipped kernel returns before its first store on a skipped step: parameters, moments and shadow keep their bits (the shadow's
    NaN fill included), at a size that runs the second trip and the tail."""
    n = ITERATION + 7
    p, m, v, grads = inputs(n, "clipped")
    from eavqa_amd.trainers.optim import bias_correction_table
    P, M, V, G = p.to(DEV), m.to(DEV), v.to(DEV), grads[BAD_STEP].to(DEV)
    sh = torch.full((n,), NAN, device=DEV, dtype=torch.bfloat16)
    st = torch.zeros(8, device=DEV, dtype=torch.int32)
    partials = torch.empty(ops.grad_sumsq_partials(n), device=DEV, dtype=torch.float64)
    kw = dict(KW)
    pre = kw.pop("grad_scale")
    ops.grad_sumsq(G, partials)
    ops.clip_plan(partials, pre, INF, bias_correction_table(kw["beta1"], kw["beta2"]).to(DEV), st)
    ops.adamw_clipped(P, G, M, V, st, shadow=sh, **kw)
    torch.cuda.synchronize()
    assert st.cpu()[4:7].tolist() == [0, 1, 1]
    assert torch.equal(bits(P.cpu()), bits(p)) and torch.equal(bits(M.cpu()), bits(m)) and torch.equal(bits(V.cpu()), bits(v))
    assert torch.isnan(sh).all()
