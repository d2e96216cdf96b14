"""References for the training-step support kernels (AdamW, LayerNorm / T5LayerNorm forward and backward, shifted cross-entropy, the
row plan and the scored-row selection): plain float64 restatements of what ``csrc/optim.hip``, ``csrc/norm.hip``, ``csrc/loss.hip``
and ``csrc/seq.hip`` document, computed from the inputs AS STORED (bf16 / fp16 tensors are widened first, never re-rounded).  CPU
only; shared by ``tests/test_train_ref_cpu.py`` (which pins every function to torch autograd / ``torch.optim.AdamW`` in float64) and
``tests/test_train_support_gpu.py``.  The input builders of the GPU cases live here too, so that the CPU file can prove them usable
(fp32 arithmetic stays inside the asserted tolerance on exactly these inputs) before any GPU run."""
import functools
import math

import torch

NEG_INF = float("-inf")


def _w(t):
    return None if t is None else t.detach().cpu().double()


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """One step of ``eavqa_adamw`` (csrc/optim.hip:67-77) -> (p, m, v) in float64: decoupled decay first, bias corrections as
    Python floats (as torch.optim.AdamW does), ``grad_scale`` applied to the gradient before anything else."""
    p, g, m, v = _w(p), _w(g) * grad_scale, _w(m), _w(v)
    p = p * (1.0 - lr * weight_decay)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adamw_step_fp32(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """The kernel's arithmetic in torch float32 (every scalar rounded to float32 where the kernel holds a float): what exact fp32
    evaluation of the formula gives, i.e. the distance from ``adamw_step`` that is the FORMAT's and not a kernel's."""
    f = lambda s: torch.tensor(s, dtype=torch.float32)
    b1, b2 = f(beta1), f(beta2)
    inv_bc1 = f(1.0 / (1.0 - float(b1) ** step))
    inv_sqrt_bc2 = f(1.0 / math.sqrt(1.0 - float(b2) ** step))
    decay = f(1.0 - float(f(lr)) * float(f(weight_decay)))
    gj = g * f(grad_scale)
    p = p * decay
    m = b1 * m + (f(1.0) - b1) * gj
    v = b2 * v + (f(1.0) - b2) * gj * gj
    denom = v.sqrt() * inv_sqrt_bc2 + f(eps)
    return p - (f(lr) * inv_bc1) * (m / denom), m, v


# the three settings of the GPU test: (first step, keyword arguments of ops.adamw, random initial moments?)
ADAMW_SETTINGS = {
    "defaults": (1, dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=0.5), False),
    "late": (1000, dict(lr=3e-4, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.1, grad_scale=1.0 / 64), True),
    "no_decay": (1, dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0), False),
}
ADAMW_STEPS = 4
ADAMW_BIG_N = 2 * 2048 * 256 * 4 + 4 * 300 + 3      # two full grid strides of float4, a partial third pass, a 3-element tail


def adamw_inputs(n, setting):
    """(p, m, v, [g_1 .. g_4]) float32 of one case; ``late`` starts from random m and non-negative v."""
    _, _, warm = ADAMW_SETTINGS[setting]
    p = rnd(n, seed=1)
    m = rnd(n, seed=2, scale=0.01) if warm else torch.zeros(n)
    v = torch.rand(n, generator=torch.Generator().manual_seed(3)) * 1e-3 if warm else torch.zeros(n)
    return p, m, v, [rnd(n, seed=10 + i) for i in range(ADAMW_STEPS)]


def adamw_run(n, setting, step_fn=adamw_step):
    """``ADAMW_STEPS`` steps of ``step_fn`` from ``adamw_inputs`` -> (p, m, v)."""
    step0, kw, _ = ADAMW_SETTINGS[setting]
    p, m, v, grads = adamw_inputs(n, setting)
    for i, g in enumerate(grads):
        p, m, v = step_fn(p, g, m, v, step0 + i, **kw)
    return p, m, v


@functools.lru_cache(maxsize=None)
def adamw_expected(n, setting):
    return adamw_run(n, setting)


# ------------------------------------------------------------------------------------------------ LayerNorm / T5LayerNorm
def layernorm_fwd(x, gamma, beta, eps):
    """-> (y, mean, rstd): biased variance, two passes."""
    x, gamma, beta = _w(x), _w(gamma), _w(beta)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    return y, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, dres):
    """-> (dx, dgamma, dbeta, abs_dgamma, abs_dbeta) from the statistics HANDED IN (the kernel gets them as float32 tensors; pass the
    same tensors): dx = dres + rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy; dgamma = sum_r dy xhat, dbeta = sum_r dy;
    the last two are sum_r |dy xhat| and sum_r |dy|, the scale of the parameter gradients' rounding bound."""
    x, dy, gamma, mean, rstd, dres = _w(x), _w(dy), _w(gamma), _w(mean), _w(rstd), _w(dres)
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy if gamma is None else dy * gamma
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres
    return dx, (dy * xhat).sum(0), dy.sum(0), (dy * xhat).abs().sum(0), dy.abs().sum(0)


def rmsnorm_fwd(x, gamma, eps):
    """T5LayerNorm -> (y, rstd): y = gamma x rsqrt(mean(x^2) + eps)."""
    x, gamma = _w(x), _w(gamma)
    rstd = 1.0 / torch.sqrt((x * x).mean(-1) + eps)
    y = x * rstd[:, None]
    return (y if gamma is None else y * gamma), rstd


def rmsnorm_bwd(x, dy, gamma, rstd, dres):
    """-> dx = dres + rstd (g - xhat mean(g xhat)), g = gamma dy, xhat = x rstd (the weight is frozen: no parameter gradient)."""
    x, dy, gamma, rstd, dres = _w(x), _w(dy), _w(gamma), _w(rstd), _w(dres)
    xhat = x * rstd[:, None]
    g = dy if gamma is None else dy * gamma
    dx = rstd[:, None] * (g - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx if dres is None else dx + dres


OFFSET_COLS = (256, 1024, 4096)


def offset_rows(rows, cols, seed=1, offset=256.0):
    """x = offset + k / 8, integer k uniform in [-8, 8]: rows whose mean dwarfs their spread.  With ``cols`` a power of two every
    intermediate of a two-pass float32 LayerNorm up to the variance sum is exact (the row sum stays below 2^24 eighths), so the
    ordinary fp32 tolerance applies; a one-pass E[x^2] - mean^2 loses the variance in the rounding of E[x^2]."""
    k = torch.randint(-8, 9, (rows, cols), generator=torch.Generator().manual_seed(seed))
    return (offset + k.double() / 8).float()


# ------------------------------------------------------------------------------------------------ cross-entropy
def row_labels_of(labels):
    """The label each logits row is scored against (csrc/loss.hip:12-16): 2-D ``labels`` [B, S] are unshifted, row b*S+s takes
    labels[b, s+1] (-100 at the last position); 1-D labels are already one per row."""
    if labels.dim() == 1:
        return labels.clone()
    out = torch.full_like(labels, -100)
    out[:, :-1] = labels[:, 1:]
    return out.reshape(-1)


def ce(logits, labels, V):
    """-> (loss, count, row_lse [rows], dlogits [rows, V]) in float64, gradient of the mean loss (gscale 1).  The kernel's label
    rule: -100 is ignored; any other label outside [0, V) makes the loss NaN and that row's gradient zero; row_lse of a row that
    is not scored is 0; no scored row at all gives 0 / 0 = NaN."""
    x = _w(logits)[:, :V]
    lab = row_labels_of(labels.cpu())
    keep = (lab >= 0) & (lab < V)
    bad = bool(((~keep) & (lab != -100)).any())
    count = int(keep.sum())
    lse = torch.logsumexp(x, dim=-1)
    safe = torch.where(keep, lab, torch.zeros_like(lab))
    row_loss = lse - x.gather(1, safe[:, None])[:, 0]
    loss = float("nan") if (bad or count == 0) else float(row_loss[keep].sum() / count)
    d = torch.exp(x - lse[:, None])
    d[torch.arange(x.shape[0]), safe] -= 1.0
    d = torch.where(keep[:, None], d / max(count, 1), torch.zeros_like(d))
    return loss, count, torch.where(keep, lse, torch.zeros_like(lse)), d


def ce_extreme_rows(V, seed=1):
    """(logits float32 [6, V], labels int64 [6]): a row times 1000, a row whose first 100 entries are -inf, a row shifted by +5000,
    a row with one 2e4 spike at its label (loss 0), and two ordinary rows."""
    x = rnd(6, V, seed=seed, scale=3.0)
    lab = torch.tensor([V // 3, V - 1, 0, V // 2, 101 % V, V - 2])
    x[0] *= 1000.0
    x[1, :100] = NEG_INF
    x[2] += 5000.0
    x[3, lab[3]] = 2e4
    return x, lab


# ------------------------------------------------------------------------------------------------ row plan / scored rows
def row_plan(mask, labels, src, pos, pack):
    """``eavqa_build_row_plan`` as loops -> (cu [B+1], src_rows, pos_rows, row_labels, flat_index), the last four of length cu[-1]:
    the kept positions (mask != 0; all of them when ``pack`` is false) of each sample in order, each with the label of the NEXT
    position of its sample (-100 at the end of a row, and everywhere when ``labels`` is None)."""
    B, S = mask.shape
    cu, src_r, pos_r, lab_r, flat = [0], [], [], [], []
    for b in range(B):
        for s in range(S):
            if pack and int(mask[b, s]) == 0:
                continue
            src_r.append(int(src[b, s]))
            pos_r.append(int(pos[b, s]))
            flat.append(b * S + s)
            lab_r.append(int(labels[b, s + 1]) if labels is not None and s + 1 < S else -100)
        cu.append(len(flat))
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return i32(cu), i32(src_r), i32(pos_r), torch.tensor(lab_r, dtype=torch.int64), i32(flat)


def select_rows(row_labels, capacity):
    """``eavqa_select_rows`` as a loop -> (sel_idx, sel_labels, count): the rows with a label >= 0 in order, the first ``capacity``
    of them stored, all of them counted."""
    idx, lab, count = [], [], 0
    for r in range(row_labels.shape[0]):
        if int(row_labels[r]) >= 0:
            if count < capacity:
                idx.append(r)
                lab.append(int(row_labels[r]))
            count += 1
    return torch.tensor(idx, dtype=torch.int32), torch.tensor(lab, dtype=torch.int64), count


def holey_mask(B, S, seed=3, empty=None, full=None):
    """int32 [B, S] mask with random holes (about 40 % zeros), optionally one sample with nothing kept and one with everything."""
    m = (torch.rand(B, S, generator=torch.Generator().manual_seed(seed)) < 0.6).int()
    if empty is not None:
        m[empty] = 0
    if full is not None:
        m[full] = 1
    return m
