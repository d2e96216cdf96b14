"""Float64 restatement of ``eavqa_ensemble_combine`` (include/eavqa.h), written from the definition: what the GPU tests compare the
kernel and the ensemble generation paths with; tests/test_ensemble_ref_cpu.py pins it to torch."""
import math

import torch

NEG_INF = float("-inf")


def normalise(weights, n):
    """The weight rule: None = 1 / n each; else n finite numbers >= 0, not all 0, divided by their sum."""
    if weights is None:
        return [1.0 / n] * n
    w = [float(x) for x in weights]
    if len(w) != n or any(not math.isfinite(x) or x < 0 for x in w) or sum(w) <= 0:
        raise ValueError(f"weights {w} for {n} members")
    total = math.fsum(w)
    return [x / total for x in w]


def member_logprobs(x):
    """float64 log_softmax of the rows of ``x`` [..., V] and their log-sum-exp [...]; a row without a finite entry is all -inf."""
    x = x.double()
    M = x.max(dim=-1, keepdim=True).values
    M = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    lse = M + torch.log(torch.exp(x - M).sum(dim=-1, keepdim=True))
    return torch.where(torch.isinf(lse), torch.full_like(x, NEG_INF), x - lse), lse.squeeze(-1)


def combine(logits, n, mode, weights=None):
    """``logits`` [B * n, V], rows ordered (question, member) -> float64 [B, V].  Only members with a weight above 0 count.  product:
    sum_i w_i lp_i[v], -inf as soon as one counted member is; mixture: m + log sum_i w_i exp(lp_i[v] - m) with m the counted maximum,
    -inf where every counted member is (no -inf - -inf is formed)."""
    w = normalise(weights, n)
    lp, _ = member_logprobs(logits)
    R, V = lp.shape
    lp = lp.view(R // n, n, V)
    counted = [i for i in range(n) if w[i] > 0]
    out = torch.empty((R // n, V), dtype=torch.float64)
    for b in range(R // n):
        rows = [lp[b, i] for i in counted]
        if mode == "product":
            acc = torch.zeros(V, dtype=torch.float64)
            for i, r in zip(counted, rows):
                acc = acc + w[i] * r                       # w > 0: a -inf stays -inf, and nothing is multiplied by 0
            out[b] = acc
        elif mode == "mixture":
            m = torch.stack(rows).max(dim=0).values
            dead = torch.isinf(m) & (m < 0)
            safe = torch.where(dead, torch.zeros_like(m), m)
            s = torch.zeros(V, dtype=torch.float64)
            for i, r in zip(counted, rows):
                s = s + w[i] * torch.exp(r - safe)
            out[b] = torch.where(dead, torch.full_like(m, NEG_INF), safe + torch.log(s))
        else:
            raise ValueError(mode)
    return out
