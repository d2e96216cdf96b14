"""Reference for gradient-norm clipping with the non-finite guard (``eavqa_grad_sumsq`` + ``eavqa_clip_plan`` + ``eavqa_adamw_clipped``,
``FusedAdamW(max_grad_norm=...)``): a float64 restatement of ``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2)`` applied
to the gradient scaled by ``pre_scale``, followed by ``_train_ref.adamw_step`` at the APPLIED step count.  A non-finite norm skips the
step: nothing changes but the skipped count (an addition to torch, GradScaler's rule for the step number).  CPU only; pinned to torch by
``tests/test_grad_clip_ref_cpu.py``, used by ``tests/test_grad_clip_gpu.py``."""
import math

import torch

import _train_ref as R


def grad_norm(g, pre_scale):
    """``pre_scale * sqrt(sum g^2)`` over the flat gradient as stored, in float64 (a Python float; nan / inf pass through)."""
    return float(pre_scale) * math.sqrt(float((R._w(g) ** 2).sum()))


def clip_coef(norm, max_norm):
    """``min(1, max_norm / (norm + 1e-6))``: clip_grad_norm_'s coefficient (``max_norm = inf`` gives 1)."""
    return min(1.0, float(max_norm) / (norm + 1e-6))


class State:
    """What the device state block carries from step to step."""

    def __init__(self, applied=0, skipped=0):
        self.applied, self.skipped, self.norm, self.skip = applied, skipped, 0.0, False


def clipped_adamw_step(p, g, m, v, state, pre_scale, max_norm, lr, beta1, beta2, eps, weight_decay):
    """One optimiser step -> (p, m, v) in float64; ``state`` is advanced in place."""
    state.norm = grad_norm(g, pre_scale)
    state.skip = not math.isfinite(state.norm)
    if state.skip:
        state.skipped += 1
        return R._w(p), R._w(m), R._w(v)
    state.applied += 1
    return R.adamw_step(p, g, m, v, state.applied, lr, beta1, beta2, eps, weight_decay, float(pre_scale) * clip_coef(state.norm, max_norm))
