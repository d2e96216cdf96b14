"""CPU: the clipping reference (tests/_clip_ref.py) is torch's: ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW`` on float64
parameters, to 1e-12 relative, over 6 optimiser steps whose gradients are scaled by 1/2 first (the accumulation scale ``fit()`` passes)
and whose norms are chosen so that some steps clip, some do not and one lands exactly on ``max_norm``.  Passes without the feature: it
pins the yardstick the GPU tests use."""
import math

import torch

import _clip_ref as C
import _train_ref as R

F64 = torch.float64
MAX_NORM, PRE = 1.0, 0.5
KW = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
# norm of the SCALED gradient per step: below, far above, exactly on, just below, just above, far below max_norm
NORMS = [0.3, 7.0, "exact", 0.999, 1.001, 1e-3]
SHAPES = [(5, 7), (11,)]
N = sum(math.prod(s) for s in SHAPES)


def close(a, b, rel=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return bool(((a - b).abs() <= rel * torch.maximum(b.abs(), torch.ones_like(b))).all())


def gradients():
    out = []
    for i, target in enumerate(NORMS):
        if target == "exact":
            g = torch.zeros(N, dtype=F64)
            g[[0, 9, 35, N - 1]] = 1.0                # scaled by 1/2: four entries of 0.5, whose norm is exactly 1.0
        else:
            g = R.rnd(N, seed=40 + i).double()
            g = g * (target / (PRE * float(g.norm())))
        out.append(g)
    return out


def test_the_chosen_norms_clip_some_steps_and_not_others():
    norms = [C.grad_norm(g, PRE) for g in gradients()]
    assert norms[2] == MAX_NORM
    coefs = [C.clip_coef(n, MAX_NORM) for n in norms]
    assert [c < 1.0 for c in coefs] == [False, True, True, False, True, False]      # (on max_norm: 1 / (1 + 1e-6) < 1, as in torch)
    assert C.clip_coef(123.0, float("inf")) == 1.0 and C.clip_coef(0.0, 1.0) == 1.0


def test_clipped_adamw_is_clip_grad_norm_then_torch_adamw():
    flat = R.rnd(N, seed=1).double()
    params, off = [], 0
    for s in SHAPES:
        n = math.prod(s)
        params.append(flat[off:off + n].clone().view(s).requires_grad_(True))
        off += n
    opt = torch.optim.AdamW(params, lr=KW["lr"], betas=(KW["beta1"], KW["beta2"]), eps=KW["eps"], weight_decay=KW["weight_decay"])
    p, m, v, state = flat.clone(), torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64), C.State()
    for g in gradients():
        off = 0
        for q in params:
            q.grad = (g[off:off + q.numel()] * PRE).view(q.shape).clone()
            off += q.numel()
        total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM, norm_type=2, error_if_nonfinite=False)
        opt.step()
        p, m, v = C.clipped_adamw_step(p, g, m, v, state, PRE, MAX_NORM, **KW)
        assert close(state.norm, total) and not state.skip
        assert close(p, torch.cat([q.detach().reshape(-1) for q in params]))
        assert close(m, torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in params]))
        assert close(v, torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params]))
    assert (state.applied, state.skipped) == (6, 0)


def test_infinite_max_norm_is_plain_adamw():
    p, m, v, state = R.rnd(N, seed=1).double(), torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64), C.State()
    q, qm, qv = p.clone(), m.clone(), v.clone()
    for t, g in enumerate(gradients(), start=1):
        p, m, v = C.clipped_adamw_step(p, g, m, v, state, PRE, float("inf"), **KW)
        q, qm, qv = R.adamw_step(q, g, qm, qv, t, grad_scale=PRE, **KW)
        assert torch.equal(p, q) and torch.equal(m, qm) and torch.equal(v, qv)


def test_a_non_finite_gradient_skips_the_step_and_keeps_the_step_number():
    grads = gradients()
    p0, m0, v0 = R.rnd(N, seed=1).double(), R.rnd(N, seed=2).double() * 0.01, R.rnd(N, seed=3).double().abs() * 1e-3
    for bad in (float("nan"), float("inf"), float("-inf")):
        state = C.State(applied=4, skipped=1)
        g = grads[0].clone()
        g[17] = bad
        p, m, v = C.clipped_adamw_step(p0, g, m0, v0, state, PRE, MAX_NORM, **KW)
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        assert (state.applied, state.skipped, state.skip) == (4, 2, True) and not math.isfinite(state.norm)
        p, m, v = C.clipped_adamw_step(p0, grads[1], m0, v0, state, PRE, MAX_NORM, **KW)
        want = R.adamw_step(p0, grads[1], m0, v0, 5, grad_scale=PRE * C.clip_coef(C.grad_norm(grads[1], PRE), MAX_NORM), **KW)
        assert (state.applied, state.skipped, state.skip) == (5, 2, False) and all(torch.equal(a, b) for a, b in zip((p, m, v), want))
