"""Reference for ``eavqa_sample_pick``: HF's three warpers restated in torch (every cumulative sum in float64), Philox4x32-10 in numpy,
the inverse CDF in index order, and the margins that say how far a case is from a decision boundary.  CPU only; shared by the CPU and
the GPU sampling tests (``tests/test_sample_ref_cpu.py`` pins the warpers to the installed transformers and Philox to Random123's
known-answer vectors)."""
import functools

import numpy as np
import torch

NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------ warpers
def warp(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (transformers generation/logits_process.py, min_tokens_to_keep 1)
    on float32 ``logits`` [rows, V]: the processed scores (float32; -inf where removed).  ``top_k`` <= 0 or >= V and ``top_p`` >= 1
    switch a filter off.  Top-p is stated as the value threshold the kernel documents: a token goes while the float64 cumulative
    probability up to and including ITS VALUE is <= 1 - top_p (equal values stand or fall together)."""
    s = (logits.float() / torch.tensor(temperature, dtype=torch.float32)).clone()
    V = s.shape[-1]
    if 0 < top_k < V:
        kth = torch.topk(s, top_k, dim=-1).values[..., -1:]
        s = s.masked_fill(s < kth, NEG_INF)
    if top_p < 1.0:
        for r in range(s.shape[0]):
            s[r] = _top_p_row(s[r], top_p)
    return s


def _top_p_row(s: torch.Tensor, top_p: float) -> torch.Tensor:
    p = torch.softmax(s.double(), dim=-1)
    vals, inv = torch.unique(s, sorted=True, return_inverse=True)              # ascending distinct values
    mass = torch.zeros(vals.shape[0], dtype=torch.float64).index_add_(0, inv, p)
    cum = mass.cumsum(0)                                                       # mass of everything <= this value
    remove = cum <= (1.0 - float(np.float32(top_p)))
    remove[-1] = False                                                         # min_tokens_to_keep = 1
    return s.masked_fill(remove[inv], NEG_INF)


def top_p_margin(logits: torch.Tensor, temperature: float, top_k: int, top_p: float) -> float:
    """Smallest |cum_j - (1 - top_p)| over the rows and the distinct values j of what top-k left (float64): how far the case is from
    the point where rounding could move the top-p boundary.  inf when top-p is off."""
    if top_p >= 1.0:
        return float("inf")
    s = warp(logits, temperature, top_k, 1.0)
    best = float("inf")
    for r in range(s.shape[0]):
        p = torch.softmax(s[r].double(), dim=-1)
        vals, inv = torch.unique(s[r], sorted=True, return_inverse=True)
        cum = torch.zeros(vals.shape[0], dtype=torch.float64).index_add_(0, inv, p).cumsum(0)
        best = min(best, float((cum[:-1] - (1.0 - float(np.float32(top_p)))).abs().min()) if cum.numel() > 1 else float("inf"))
    return best


# ------------------------------------------------------------------------------------------------ inverse CDF
def probs(processed_row: torch.Tensor) -> torch.Tensor:
    """float64 probabilities of one processed row (0 where removed)."""
    return torch.softmax(processed_row.double(), dim=-1)


def cdf(processed_row: torch.Tensor) -> torch.Tensor:
    return probs(processed_row).cumsum(0)


def inverse_cdf(processed_row: torch.Tensor, u: float) -> int:
    """The smallest index i with sum_{j <= i} p_j > u (probabilities normalised over the kept tokens, float64); the last token with
    mass when rounding leaves none."""
    p = probs(processed_row)
    hit = (p.cumsum(0) > float(u)) & (p > 0)
    if bool(hit.any()):
        return int(hit.nonzero()[0])
    return int((p > 0).nonzero()[-1])


def cdf_margin(processed_row: torch.Tensor, u: float) -> float:
    """Distance of ``u`` to the nearest boundary of the CDF (float64, in probability)."""
    return float((cdf(processed_row) - float(u)).abs().min())


def midpoint_uniform(processed_row: torch.Tensor, i: int) -> np.float32:
    """The middle of token i's CDF interval, rounded to float32."""
    c = cdf(processed_row)
    lo = float(c[i - 1]) if i > 0 else 0.0
    return np.float32(0.5 * (lo + float(c[i])))


# ------------------------------------------------------------------------------------------------ Philox4x32-10
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Random123 ``philox4x32_10``: 4 counter words, 2 key words -> 4 output words (python ints)."""
    c0, c1, c2, c3 = [int(x) & _MASK for x in counter]
    k0, k1 = [int(x) & _MASK for x in key]
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def philox_uniform(seed: int, step: int, row: int) -> np.float32:
    """The uniform ``eavqa_sample_pick`` uses for (seed, step, row): first word of Philox4x32-10 with key (seed lo, seed hi) and counter
    (step lo, step hi, row, 0), as (x >> 8) * 2^-24."""
    x = philox4x32_10((step & _MASK, (step >> 32) & _MASK, row, 0), (seed & _MASK, (seed >> 32) & _MASK))[0]
    return np.float32((x >> 8) * 2.0 ** -24)


def philox_uniforms(seed: int, step: int, rows: int) -> np.ndarray:
    return np.array([philox_uniform(seed, step, b) for b in range(rows)], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the fixed cases of the GPU tests
SHAPES = [(1, 7, 7), (3, 64, 64), (5, 1000, 1001), (3, 32128, 32192), (1, 50272, 50272)]        # (B, V, ld)
TEMPERATURES = (1.0, 0.7, 2.0)
TOP_KS = (0, 1, 2, 50, "V+5")
TOP_PS = (1.0, 0.9, 0.5, 1e-6)


def _top_ks(V: int):
    return [V + 5 if k == "V+5" else k for k in TOP_KS]


LIVE = 40          # finite columns per row of a fixed case with V >= 1000 (see case_logits)


def _row_margin(row: torch.Tensor, V: int) -> float:
    x = row[None]
    return min(top_p_margin(x, t, k, p) for t in TEMPERATURES for k in sorted(set(_top_ks(V))) for p in TOP_PS)


@functools.lru_cache(maxsize=None)
def _case_logits(B: int, V: int, seed: int) -> torch.Tensor:
    rows = []
    for b in range(B):
        for attempt in range(1000):
            g = torch.Generator().manual_seed(((1000 * V + b) * 1000 + seed) * 1000 + attempt)
            x = torch.randn(V, generator=g) * 3
            if V >= 1000:
                live = torch.randperm(V, generator=g)[:LIVE - 2].tolist() + [V - 1, V - 1 - (V % 4096) // 2]   # the tail chunk included
                keep = torch.zeros(V, dtype=torch.bool)
                keep[live] = True
                x[~keep] = NEG_INF
            else:
                x[torch.randperm(V, generator=g)[:max(1, V // 9)]] = NEG_INF
                x[(3 * b + 1) % V] = NEG_INF
            last = int(torch.isfinite(x).nonzero()[-1])
            if _row_margin(x, V) >= 1.5e-4 and float(torch.softmax(x.double(), -1)[last]) >= 1e-4:
                break
        else:
            raise AssertionError("no seed gives the top-p margin")
        rows.append(x)
    return torch.stack(rows)


def case_logits(B: int, V: int, seed: int = 0) -> torch.Tensor:
    """The logits of a fixed case: seeded randn * 3 with some columns at -inf.  HOW MANY is decided by the margin the exact tests
    need: a top-p boundary can only lie 1e-4 away from every cumulative probability when the token that straddles it weighs more than
    2e-4, and in ascending order the boundary of top_p = 0.9 sits among the LIGHTEST tokens - at temperature 2 that allows a few dozen
    finite columns, not thousands.  So rows of V >= 1000 keep ``LIVE`` finite columns spread over the whole row (the last column and the
    partial tail chunk included) and smaller rows lose a ninth; per row the first seed whose margin (float64, reference only) is
    >= 1.5e-4 over the whole (temperature, top_k, top_p) grid is taken - and whose last finite column weighs >= 1e-4 at temperature 1, so
    that the uniform 1 - 2^-24 has to land on it.  Dense rows are covered by :func:`dense_logits` with a band."""
    return _case_logits(B, V, seed).clone()


def dense_logits(B: int, V: int, seed: int = 0) -> torch.Tensor:
    """randn * 3 in every column but a few at -inf: what an LM head produces.  A top-p boundary then lies within ~1e-5 of some token's
    cumulative probability, so the mask is compared outside :func:`top_p_band` only."""
    g = torch.Generator().manual_seed(77 * V + B + seed)
    x = torch.randn(B, V, generator=g) * 3
    x[:, torch.randperm(V, generator=g)[:17]] = NEG_INF
    return x


def top_p_band(logits_row: torch.Tensor, temperature: float, top_k: int, top_p: float, width: float) -> torch.Tensor:
    """bool [V]: tokens whose float64 cumulative probability (ascending by value, after top-k) lies within ``width`` of 1 - top_p."""
    s = warp(logits_row[None], temperature, top_k, 1.0)[0]
    p = torch.softmax(s.double(), dim=-1)
    vals, inv = torch.unique(s, sorted=True, return_inverse=True)
    cum = torch.zeros(vals.shape[0], dtype=torch.float64).index_add_(0, inv, p).cumsum(0)
    near = (cum - (1.0 - float(np.float32(top_p)))).abs() < width
    near[-1] = False
    return near[inv]


def filter_cases():
    """Every (B, V, ld, temperature, top_k, top_p) of the filter test."""
    for B, V, ld in SHAPES:
        for t in TEMPERATURES:
            for k in TOP_KS:
                for p in TOP_PS:
                    yield B, V, ld, t, (V + 5 if k == "V+5" else k), p
