"""Exact per-key probes for the attention kernels: case table, input builders, float64 reference and the acceptance check.

Random data averages a one-key visibility error away (a softmax over n keys moves by about 1 / n); these inputs are built so that
every (query, key) pair shows up on its own in some output element, and the bound follows from bf16 rounding alone:

  Probe A (read-out)   q = 0, so every score is zero (or the relative-position bias alone) and P is uniform (or the softmax of the
                       bias) over the visible keys.  Indicator matrices in V, dO and K read P out element by element: through the
                       output, through dV (column j of P) and through dQ (scale * P_ij * (a_j - sum_j P_ij a_j), signs a_j).
  Probe B (selection)  keys carry the +/-1 binary code of j + 1, a query is 32 code(t1) or 16 (code(t1) + code(t2)) with t2 the
                       neighbour of t1 across the lowest bit of j + 1 (pairs (63, 64), (127, 128): across key-tile edges).  At scale 1
                       the chosen key (or pair) wins by 64 in the exponent: P is one-hot or (0.5, 0.5), O copies or averages V rows.

No GPU is needed to import this file; tests/test_attention_probe_cpu.py checks the probes themselves and
tests/test_attention_probe_gpu.py runs them through the kernels.  The second half of the file carries the same two probes over to
the shared-prompt decode step, the two-segment merge and the scoring flow (tests/test_shared_attention_probe_gpu.py).

Layout: q / dO / o / dq are [B, Sq, H, hd], k / v / dk / dv are [B, Sk, H, hd], P is [B, H, Sq, Sk], float64 on the CPU.
"""
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch

EPS = {torch.bfloat16: 2.0 ** -8, torch.float32: 1e-5}      # per-summand relative rounding: two bf16 half-ulps / the project's fp32 tolerance
ABS_FLOOR = 1e-6
ZERO = 1e-30                                                # what an invisible key may read in Probe A
LSE_TOL = 1e-3                                              # the bound test_attention_decode_step holds
TILE = 64
CODE_BITS = 10


# ------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    B: int
    H: int
    Sq: int
    Sk: int
    hd: int
    causal: bool
    mask: str                                   # "right" | "left" | "holes" | "none" | "packed"
    buckets: Optional[str] = None               # rel route: "bi" (bidirectional) | "one" (one-sided); None = no bias
    empty_rows: int = 0                         # query rows without a visible key (only "left" under a causal mask has any)
    lens: Optional[Tuple[int, ...]] = None      # packed rows: the samples' lengths (B = len(lens), Sq = Sk = max(lens))
    note: str = ""

    @property
    def id(self):
        s = f"{self.B}x{self.H}x{self.Sq}x{self.Sk}x{self.hd}-{'causal' if self.causal else 'full'}-{self.mask}"
        if self.buckets:
            s += "-" + self.buckets
        if self.lens:
            s += "-" + "_".join(map(str, self.lens))
        return s


PLAIN_CASES = [
    Case(2, 2, 17, 17, 64, True, "right", note="FAST=false, one fragment + 1, fused64 backward (path 4: the padded kernel)"),
    Case(2, 2, 64, 64, 64, True, "left", empty_rows=14, note="exactly one tile"),
    Case(2, 2, 65, 65, 64, False, "holes", note="second tile one row deep, NW 5"),
    Case(2, 1, 129, 129, 128, True, "left", empty_rows=75, note="a fully masked interior tile, dkv LDS opt-in"),
    Case(2, 2, 170, 170, 64, False, "right", note="NW 6"),
    Case(1, 2, 70, 200, 80, True, "holes", note="two query tiles, off = 130, padded head chunk"),
    Case(2, 2, 100, 100, 96, False, "left", note="NW 8"),
    Case(2, 1, 40, 40, 200, False, "holes", note="wide one-tile kernels; bf16 only"),
    Case(2, 2, 20, 37, 16, True, "holes", note="VALU only; fp32 and bf16"),
]
RESIDENT_CASES = [Case(1, 2, N, N, 64, False, "none", note="K/V-resident forward: every P entry is 1 / N") for N in (65, 97, 257)]
REL_CASES = [
    Case(2, 2, 170, 170, 64, False, "right", "bi", note="NW 6, bias_tile plus a general tile"),
    Case(1, 2, 129, 129, 64, True, "none", "one", note="bias_tile below the diagonal"),
    Case(2, 2, 100, 100, 128, False, "left", "bi", note="NW 8"),
    Case(2, 2, 5, 150, 64, True, "none", "one", note="off != 0 with a bias"),
    Case(2, 3, 9, 9, 80, False, "holes", "bi", note="small, ragged head chunk"),
]
# A decode step's newest key (Sk - 1) is the token itself and always visible: a left pad is cut to Sk - 1 keys (Sk = 1: none).
DECODE_CASES = [Case(2, 3, 1, Sk, hd, True, mask, note="decode step") for Sk in (1, 64, 65, 200) for hd in (64, 80, 128) for mask in ("left", "holes")]
DECODE_REL_CASES = [Case(2, 2, 1, Sk, 64, True, mask, "one", note="decode step from partial sums, self-attention form")
                    for Sk in (1, 65, 170) for mask in ("none", "holes")]
PACKED_CASES = [
    Case(4, 2, 70, 70, 64, True, "packed", lens=(70, 1, 64, 17), note="streamed forward, dQ + dK/dV pair"),
    Case(4, 2, 64, 64, 64, True, "packed", lens=(64, 49, 16, 1), note="fused backward (paths 0 and 4)"),
]
ALL_CASES = PLAIN_CASES + RESIDENT_CASES + REL_CASES + DECODE_CASES + DECODE_REL_CASES + PACKED_CASES


# ------------------------------------------------------------------------------------------------------------------- masks, bias
def key_mask(case: Case) -> Optional[torch.Tensor]:
    """int32 [B, Sk] (1 = visible), or None."""
    B, Sk = case.B, case.Sk
    j = torch.arange(Sk)[None]
    if case.mask == "none":
        return None
    if case.mask == "right":
        lens = torch.tensor([Sk if b == 0 else max(1, Sk - 3 * b - 1) for b in range(B)])
        return (j < lens[:, None]).int()
    if case.mask == "packed":
        return (j < torch.tensor(case.lens)[:, None]).int()
    if case.mask == "left":
        pads = [5, 70 if Sk >= 129 else 9] + [3 * b for b in range(2, B)]
        pads = torch.tensor([min(p, Sk - 1) for p in pads[:B]])
        return (j >= pads[:, None]).int()
    if case.mask == "holes":
        g = torch.Generator().manual_seed(1000 + 7 * Sk + case.hd)
        km = (torch.rand(B, Sk, generator=g) > 0.3).int()
        km[:, Sk - 1] = 1
        return km
    raise ValueError(case.mask)


def visible(case: Case, km: Optional[torch.Tensor], diag: int = 0) -> torch.Tensor:
    """bool [B, 1, Sq, Sk]: key j is visible to query i (which sits at position i + Sk - Sq).  ``diag`` moves the causal diagonal."""
    keep = torch.ones(case.B, 1, case.Sq, case.Sk, dtype=torch.bool)
    if km is not None:
        keep = keep & (km != 0)[:, None, None, :]
    if case.causal:
        i, j = torch.arange(case.Sq)[:, None], torch.arange(case.Sk)[None, :]
        keep = keep & (j <= i + (case.Sk - case.Sq) + diag)[None, None]
    return keep


def rows_checked(case: Case, keep: torch.Tensor) -> torch.Tensor:
    """bool [B, Sq]: the query rows that exist and see a key.  The others get dO = 0 and their output is only asserted finite."""
    ok = keep.any(-1)[:, 0]
    if case.lens is not None:
        ok = ok & (torch.arange(case.Sq)[None] < torch.tensor(case.lens)[:, None])
    return ok


def relative_bucket(rel: torch.Tensor, bidirectional: bool, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """T5's bucket of a relative position (key - query), written out here so that the probes do not lean on the package."""
    out = torch.zeros_like(rel)
    if bidirectional:
        num_buckets //= 2
        out = out + (rel > 0).long() * num_buckets
        rel = rel.abs()
    else:
        rel = (-rel).clamp(min=0)
    max_exact = num_buckets // 2
    large = max_exact + (torch.log(rel.clamp(min=1).float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).long()
    return out + torch.where(rel < max_exact, rel, large.clamp(max=num_buckets - 1))


def bucket_values(H: int) -> torch.Tensor:
    """float32 [H, 32]: per head 32 different multiples of 1/8 in [-4, 4], another draw per head.  (65 such values exist, so the
    entries differ per bucket - which is per offset within 8 positions of the diagonal - not per offset of a long row.)"""
    rows = [(torch.randperm(65, generator=torch.Generator().manual_seed(100 + h))[:32].float() - 32.0) / 8.0 for h in range(H)]
    t = torch.stack(rows)
    assert all(not torch.equal(t[a], t[b]) for a in range(H) for b in range(a))
    return t


REL_MARGIN = 1          # spare columns either side of the table, so that a test can read it one offset off


def rel_table(case: Case):
    """(float32 [H, 2 Sk - 1 + 2 REL_MARGIN], rel_zero): element [h, (key - query) + rel_zero] is head h's bias at that offset."""
    zero = case.Sk - 1 + REL_MARGIN
    off = torch.arange(-zero, zero + 1)
    return bucket_values(case.H)[:, relative_bucket(off, case.buckets == "bi")].contiguous(), zero


def bias_matrix(case: Case, shift: int = 0) -> Optional[torch.Tensor]:
    """float64 [1, H, Sq, Sk] or None.  ``shift`` reads the table that many columns off."""
    if case.buckets is None:
        return None
    rel, zero = rel_table(case)
    i, j = torch.arange(case.Sq)[:, None], torch.arange(case.Sk)[None, :]
    return rel[:, j - (i + case.Sk - case.Sq) + zero + shift].double()[None]


# ------------------------------------------------------------------------------------------------------------------- reference
class Ref(NamedTuple):
    p: torch.Tensor
    lse: torch.Tensor                           # [B, H, Sq]
    val: dict                                   # "o", "dq", "dk", "dv" (and "ds", the score gradient, [B, H, Sq, Sk])
    mag: dict                                   # their absolute companions: the same contractions over |P|, |dS|, |q|, |k|, |v|, |dO|


def _bf16(x):
    return x.to(torch.bfloat16).double()


def reference(q, k, v, do, keep, bias, scale, fwd: Optional[Ref] = None, rnd=None) -> Ref:
    """float64 attention forward and backward, written out (no autograd) so that every gradient comes with its absolute companion.
    Rows of ``keep`` without a visible key get P = 0.  ``fwd``: take the log-sum-exp and the output from that forward and rebuild
    P = exp(s - lse) from them, as a backward kernel does (so a backward with a different visible set than its forward can be modelled).
    ``rnd``: round P, dS and every output with it (the bf16 emulation)."""
    rnd = rnd or (lambda x: x)
    B, Sq, H, hd = q.shape
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    if bias is not None:
        s = s + bias
    keep = keep.expand(B, H, Sq, k.shape[1])
    some = keep.any(-1, keepdim=True)
    if fwd is None:
        m = torch.where(keep, s, torch.full_like(s, -math.inf)).amax(-1, keepdim=True)
        m = torch.where(some, m, torch.zeros_like(m))
        e = torch.where(keep, torch.exp(s - m), torch.zeros_like(s))
        l = e.sum(-1, keepdim=True)
        p = e / torch.where(some, l, torch.ones_like(l))
        lse = (m + torch.log(torch.where(some, l, torch.ones_like(l))))[..., 0]
    else:
        lse = fwd.lse
        p = torch.where(keep & some, torch.exp(torch.where(keep, s, torch.zeros_like(s)) - lse[..., None]), torch.zeros_like(s))
    pr = rnd(p)
    val = {"o": rnd(torch.einsum("bhij,bjhd->bihd", pr, v))}
    mag = {"o": torch.einsum("bhij,bjhd->bihd", p, v.abs())}
    if do is not None:
        o_seen = fwd.val["o"] if fwd is not None else val["o"]
        dp = torch.einsum("bihd,bjhd->bhij", do, v)
        dp_mag = torch.einsum("bihd,bjhd->bhij", do.abs(), v.abs())
        delta = (do * o_seen).sum(-1).permute(0, 2, 1)[..., None]
        delta_mag = (p * dp_mag).sum(-1, keepdim=True)
        ds = rnd(pr * (dp - delta))
        ds_mag = p * (dp_mag + delta_mag)
        val["dq"] = rnd(scale * torch.einsum("bhij,bjhd->bihd", ds, k))
        val["dk"] = rnd(scale * torch.einsum("bhij,bihd->bjhd", ds, q))
        val["dv"] = rnd(torch.einsum("bhij,bihd->bjhd", pr, do))
        mag["dq"] = scale * torch.einsum("bhij,bjhd->bihd", ds_mag, k.abs())
        mag["dk"] = scale * torch.einsum("bhij,bihd->bjhd", ds_mag, q.abs())
        mag["dv"] = torch.einsum("bhij,bihd->bjhd", p, do.abs())
        val["ds"] = ds
    return Ref(p, lse, val, mag)


# ------------------------------------------------------------------------------------------------------------------- probes
class Probe(NamedTuple):
    name: str
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    do: Optional[torch.Tensor]                  # None: forward only
    scale: float
    exact_zero: bool                            # Probe A: an element whose absolute companion is zero must read |x| <= ZERO

    @property
    def outputs(self):
        return ("o",) if self.do is None else ("o", "dq", "dk", "dv")


def _randn_bf16(shape, seed):
    return _bf16(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def _ternary(shape, seed):
    return torch.randint(-1, 2, shape, generator=torch.Generator().manual_seed(seed)).double()


def _indicator(B, S, H, hd, c):
    """[B, S, H, hd]: 1 where s == c hd + d."""
    x = torch.zeros(B, S, H, hd, dtype=torch.float64)
    n = min(hd, S - c * hd)
    idx = torch.arange(n)
    x[:, c * hd + idx, :, idx] = 1.0
    return x


def probe_a_forward(case: Case):
    """q = 0, V = (1 + h) where key == c hd + d: output element (i, h, d) of pass c is (1 + h) P[b, h, i, c hd + d]."""
    B, H, Sq, Sk, hd = case.B, case.H, case.Sq, case.Sk, case.hd
    heads = (1.0 + torch.arange(H, dtype=torch.float64))[None, None, :, None]
    for c in range(-(-Sk // hd)):
        yield Probe(f"A.fwd[{c}]", torch.zeros(B, Sq, H, hd, dtype=torch.float64), _randn_bf16((B, Sk, H, hd), 21),
                    _indicator(B, Sk, H, hd, c) * heads, None, hd ** -0.5, True)


def probe_a_backward(case: Case, ok: torch.Tensor):
    """dK/dV: q = 0, V = 0, dO = query indicators: dV[j, h, d] of pass c is P[b, h, c hd + d, j].
    dQ: q = 0, K = key indicators, V[..., 0] = a_j, dO = e_0: dQ[i, h, d] of pass c is scale P_ij (a_j - sum_j P_ij a_j), j = c hd + d."""
    B, H, Sq, Sk, hd = case.B, case.H, case.Sq, case.Sk, case.hd
    zq, rows = torch.zeros(B, Sq, H, hd, dtype=torch.float64), ok[:, :, None, None].double()
    for c in range(-(-Sq // hd)):
        yield Probe(f"A.dkv[{c}]", zq, _randn_bf16((B, Sk, H, hd), 22), torch.zeros(B, Sk, H, hd, dtype=torch.float64),
                    _indicator(B, Sq, H, hd, c) * rows, hd ** -0.5, True)
    v = torch.zeros(B, Sk, H, hd, dtype=torch.float64)
    v[..., 0] = (2.0 * torch.randint(0, 2, (B, Sk, H), generator=torch.Generator().manual_seed(23)) - 1.0).double()
    do = torch.zeros(B, Sq, H, hd, dtype=torch.float64)
    do[..., 0] = 1.0
    for c in range(-(-Sk // hd)):
        yield Probe(f"A.dq[{c}]", zq, _indicator(B, Sk, H, hd, c), v, do * rows, hd ** -0.5, True)


def code(n: torch.Tensor) -> torch.Tensor:
    """+/-1 binary code of n in CODE_BITS features."""
    return (((n[..., None] >> torch.arange(CODE_BITS)) & 1) * 2 - 1).double()


def select_targets(keep_bi: torch.Tensor, i: int):
    """The keys query row i asks for: (t1, t2 or None).  Cycles last / first / middle / (7 i) mod n visible key; t2 is t1's neighbour across
    the lowest bit of key + 1, used whenever it is visible too."""
    vis = torch.nonzero(keep_bi)[:, 0].tolist()
    n = len(vis)
    t1 = vis[(n - 1, 0, n // 2, (7 * i) % n)[i % 4]]
    t2 = ((t1 + 1) ^ 1) - 1
    return t1, (t2 if 0 <= t2 < keep_bi.numel() and bool(keep_bi[t2]) else None)


def probe_b(case: Case, keep: torch.Tensor, ok: torch.Tensor, backward: bool = True, target=None) -> Probe:
    """Selection at scale 1.  ``target(b, i, visible keys)`` overrides the cycle with a one-hot target (decode steps)."""
    B, H, Sq, Sk, hd = case.B, case.H, case.Sq, case.Sk, case.hd
    assert hd >= CODE_BITS and Sk + 1 < 2 ** CODE_BITS
    k = torch.zeros(B, Sk, H, hd, dtype=torch.float64)
    k[..., :CODE_BITS] = code(torch.arange(Sk) + 1)[None, :, None, :]
    q = torch.zeros(B, Sq, H, hd, dtype=torch.float64)
    for b in range(B):
        for i in range(Sq):
            if not ok[b, i]:
                continue
            if target is not None:
                t1, t2 = target(b, i, torch.nonzero(keep[b, 0, i])[:, 0].tolist()), None
            else:
                t1, t2 = select_targets(keep[b, 0, i], i)
            row = 32.0 * code(torch.tensor(t1 + 1)) if t2 is None else 16.0 * (code(torch.tensor(t1 + 1)) + code(torch.tensor(t2 + 1)))
            q[b, i, :, :CODE_BITS] = row
    do = _ternary((B, Sq, H, hd), 32) * ok[:, :, None, None].double() if backward else None
    return Probe("B", q, k, _ternary((B, Sk, H, hd), 31), do, 1.0, False)


DECODE_PICKS = {                                # a decode step's one-hot targets: the newest key, the first visible one, the tile edge
    "last": lambda b, i, vis: vis[-1],
    "first": lambda b, i, vis: vis[0],
    "edge": lambda b, i, vis: max([j for j in vis if j <= TILE] or vis[:1]),        # key 64, or the visible key closest below it
}


def probes(case: Case, keep: torch.Tensor, ok: torch.Tensor, backward: bool = True):
    """Every probe of a case.  Tiled cases: Probe A forward, Probe B, Probe A through the gradients.  A decode step (Sq = 1): Probe A
    forward, then Probe B one-hot on DECODE_PICKS - or, from partial sums with a bias, Probe A alone."""
    yield from probe_a_forward(case)
    if case.Sq == 1:
        if case.buckets is None:
            for name, pick in DECODE_PICKS.items():
                yield probe_b(case, keep, ok, backward=False, target=pick)._replace(name="B." + name)
        return
    yield probe_b(case, keep, ok, backward)
    if backward:
        yield from probe_a_backward(case, ok)


# ------------------------------------------------------------------------------------------------------------------- acceptance
def check(got: dict, ref: Ref, dtype, ok: torch.Tensor, exact_zero: bool, names=None, what: str = "") -> float:
    """|got - want| <= EPS (abs_companion + |want|) + 1e-6 elementwise for every tensor of ``got`` ("o", "dq", "dk", "dv"; "lse" within
    LSE_TOL); rows of o / dq / lse outside ``ok`` only finite; ``exact_zero``: where the companion is zero, |got| <= ZERO.
    Returns the worst error / bound; raises AssertionError naming the worst element."""
    worst = 0.0
    rows = ok[:, :, None, None]
    for name in names or got.keys():
        g = got[name].double()
        if name == "lse":
            g = torch.where(ok[:, None, :], g, torch.zeros_like(g))
        assert torch.isfinite(g).all(), f"{what} {name}: non-finite values"
        if name == "lse":
            err, bound = (g - ref.lse).abs() * ok[:, None, :], torch.full_like(g, LSE_TOL)
        else:
            want, mag = ref.val[name], ref.mag[name]
            err, bound = (g - want).abs(), EPS[dtype] * (mag + want.abs()) + ABS_FLOOR
            if name in ("o", "dq"):
                err = err * rows
            if exact_zero:
                leak = g.abs() * (mag == 0) * (rows if name in ("o", "dq") else 1.0)
                assert leak.max().item() <= ZERO, f"{what} {name}: {leak.max().item():.3g} where nothing is visible, at {_where(leak)}"
        ratio = err / bound
        r = ratio.max().item()
        assert r <= 1.0, f"{what} {name}: error / bound = {r:.3f} at {_where(ratio)} (error {err.flatten()[ratio.argmax()].item():.4g})"
        worst = max(worst, r)
    return worst


def _where(x):
    return tuple(int(t) for t in torch.unravel_index(x.argmax(), x.shape))


# ------------------------------------------------------------------------------------------------------------------- mutations
MUTATIONS = ("diag+1", "diag-1", "last_key_visible", "last_key_hidden", "tile_mask_late", "tile_first_key_dropped", "bias+1", "bias-1")


def mutate(case: Case, km: Optional[torch.Tensor], name: str):
    """The visible set and bias of a kernel that is wrong in one of the ways a tiled kernel goes wrong: (keep, bias)."""
    m = km.clone() if km is not None else torch.ones(case.B, case.Sk, dtype=torch.int32)
    diag, shift = 0, 0
    if name in ("diag+1", "diag-1"):
        diag = (1 if name == "diag+1" else -1) if case.causal else 0
    elif name == "last_key_visible":
        m[:, case.Sk - 1] = 1
    elif name == "last_key_hidden":
        m[:, case.Sk - 1] = 0
    elif name == "tile_mask_late":                           # the first 64-key tile whose mask changes when read one position late
        for t0 in range(0, case.Sk, TILE):
            j = torch.arange(t0, min(t0 + TILE, case.Sk))
            late = m[:, (j - 1).clamp(min=0)]
            if not torch.equal(late, m[:, j]):
                m[:, j] = late
                break
    elif name in ("bias+1", "bias-1"):
        shift = 1 if name == "bias+1" else -1
    keep = visible(case, m, diag)
    if name == "tile_first_key_dropped":                     # ... for the last 16-row fragment of queries
        keep = keep.clone()
        keep[:, :, 16 * ((case.Sq - 1) // 16):, ::TILE] = False
    return keep, bias_matrix(case, shift)


# =================================================================================================================== shared prompt
# eavqa_attention_decode_shared: B prompts x G rows, one decode step.  A call is modelled as an ordinary case of B G query rows with
# Sq = 1 over the key axis [prompt 0..S0-1 | tail 0..t]; the physical buffers (prompt caches with spare rows, tails with spare slots,
# a mask with a row stride beyond S0) are built from a probe by shared_buffers, and shared_gather reads them back the way a kernel
# does - or the way a kernel that is wrong in one index does (SHARED_MUTATIONS).
GARBAGE = 3.0                                   # what spare cache rows and tail slots hold: finite, and wrong if read
SH_WPH, SH_U = 2, 8                             # csrc/attention_decode_shared.hip (tests/test_attention_probe_cpu.py parses them)


def shared_lpk(dtype: str, hd: int) -> int:
    """Lanes per key of the template form a (dtype, hd) pair launches."""
    return {("bf16", True): 8, ("bf16", False): 16, ("fp32", True): 16, ("fp32", False): 32}[dtype, hd <= 64]


@dataclass(frozen=True)
class SharedCase:
    dtype: str                                  # "bf16" | "fp32"
    G: int
    H: int
    S0: int
    n: int                                      # t + 1 tail keys
    t_max: int
    hd: int
    mask: str                                   # "lh": left pad on prompt 0, holes on prompt 1 | "all1": prompt 1 fully masked | "none"

    B = 2                                       # prompts (a class constant: every case has two)

    @property
    def kpi(self):
        return 64 // shared_lpk(self.dtype, self.hd)

    @property
    def step(self):                             # prompt keys per batch of a head
        return self.kpi * SH_WPH * SH_U

    @property
    def tb(self):                               # tail keys per row and batch
        return (SH_U // self.G) * SH_WPH * self.kpi

    @property
    def case(self) -> Case:
        return Case(self.B * self.G, self.H, 1, self.S0 + self.n, self.hd, True, "shared")

    @property
    def bits(self):
        return min(CODE_BITS, self.hd)

    @property
    def torch_dtype(self):
        return torch.bfloat16 if self.dtype == "bf16" else torch.float32

    @property
    def id(self):
        return f"{self.dtype}-G{self.G}-H{self.H}-S{self.S0}-n{self.n}of{self.t_max}-hd{self.hd}-{self.mask}"


def _shared_table(dtype: str, wide: bool):
    """15 cases of one template form: S0 over the prompt batch edges, t + 1 over the tail batch edges of the case's G, every value of an
    axis with at least two values of each other axis (test_shared_table_covers_every_pair_of_axes holds it to that)."""
    hds = (80, 128) if wide else (8, 40, 64)
    gs = (1, 2, 3, 5, 8)
    out = []
    for i in range(15):
        G = gs[(2 * i + i // 5) % 5]
        hd = hds[i % len(hds)]
        form = SharedCase(dtype, G, 4, 1, 1, 1, hd, "lh")
        step, tb = form.step, form.tb
        S0 = (1, step - 1, step, step + 1, 2 * step + 1)[3 * i % 5]
        n = (1, tb - 1, tb, tb + 1)[(i + i // 2) % 4]
        if hd == 8 and S0 + n + 2 >= 2 ** 8:                # Probe B codes keys in min(CODE_BITS, hd) bits
            hd = 40
        t_max = n if (i // 2) % 2 == 0 else 256
        out.append(SharedCase(dtype, G, (4, 5)[(i // 5) % 2], S0, n, t_max, hd, {3: "all1", 7: "none"}.get(i, "lh")))
    return out


SHARED_CASES = [c for dtype in ("bf16", "fp32") for wide in (False, True) for c in _shared_table(dtype, wide)]


def shared_mask(sc: SharedCase) -> Optional[torch.Tensor]:
    """int32 [B, S0 + 3] with ones behind S0, or None."""
    if sc.mask == "none":
        return None
    m = torch.ones(sc.B, sc.S0 + 3, dtype=torch.int32)
    m[0, :min(5, sc.S0 - 1)] = 0
    if sc.mask == "all1":
        m[1, :sc.S0] = 0
    else:
        g = torch.Generator().manual_seed(2000 + 7 * sc.S0 + sc.hd)
        m[1, :sc.S0] = (torch.rand(sc.S0, generator=g) > 0.3).int()
        m[1, sc.S0 - 1] = 1
    return m


def shared_keep(sc: SharedCase) -> torch.Tensor:
    """bool [B G, 1, 1, S0 + n]: prompt mask of b, then n ones."""
    m = shared_mask(sc)
    keep = torch.ones(sc.B, sc.S0 + sc.n, dtype=torch.bool)
    if m is not None:
        keep[:, :sc.S0] = m[:, :sc.S0] != 0
    return keep.repeat_interleave(sc.G, 0)[:, None, None, :]


def _share_prompt(x, sc: SharedCase):
    """The prompt part of row (b, g) becomes that of row (b, 0)."""
    x[:, :sc.S0] = x[::sc.G, :sc.S0].repeat_interleave(sc.G, 0)
    return x


def shared_probe_a(sc: SharedCase):
    """q = 0; V of pass c marks key c hd + d of the concatenated axis, times (1 + h) in the prompt and (1 + h)(1 + g) in row g's tail."""
    case = sc.case
    R, H, Sk, hd = case.B, case.H, case.Sk, case.hd
    factor = (1.0 + torch.arange(H, dtype=torch.float64))[None, None, :, None].repeat(R, Sk, 1, 1)
    factor[:, sc.S0:] *= (1.0 + (torch.arange(R) % sc.G).double())[:, None, None, None]
    k = _share_prompt(_randn_bf16((R, Sk, H, hd), 21), sc)
    for c in range(-(-Sk // hd)):
        yield Probe(f"A.fwd[{c}]", torch.zeros(R, 1, H, hd, dtype=torch.float64), k, _indicator(R, Sk, H, hd, c) * factor, None, hd ** -0.5, True)


SHARED_PICKS = ("first prompt", "last prompt", "edge - 1", "edge", "tail 0", "tail t - 1", "tail t")


def shared_target(sc: SharedCase, keep_r: torch.Tensor, pick: str) -> int:
    """The key (concatenated axis) a pick names for a row whose visible set is ``keep_r`` [S0 + n]; without a visible prompt key the
    prompt picks fall on tail key t."""
    vis = torch.nonzero(keep_r[:sc.S0])[:, 0].tolist()
    t = sc.n - 1
    if pick.startswith("tail"):
        return sc.S0 + {"tail 0": 0, "tail t - 1": max(t - 1, 0), "tail t": t}[pick]
    if not vis:
        return sc.S0 + t
    if pick in ("edge - 1", "edge"):
        e = sc.step - (pick == "edge - 1")
        return max([j for j in vis if j <= e] or vis[:1])
    return vis[0] if pick == "first prompt" else vis[-1]


def shared_probe_b(sc: SharedCase):
    """Keys carry code(j + 1) over the concatenated axis; row r of probe p asks for pick (r + p R) mod 7, so the rows of a prompt ask
    for different keys and every pick is asked for in every case."""
    case = sc.case
    R, H, Sk, hd, bits = case.B, case.H, case.Sk, case.hd, sc.bits
    assert Sk + 1 < 2 ** bits
    keep = shared_keep(sc)
    feat = lambda n: (((n[..., None] >> torch.arange(bits)) & 1) * 2 - 1).double()
    k = torch.zeros(R, Sk, H, hd, dtype=torch.float64)
    k[..., :bits] = feat(torch.arange(Sk) + 1)[None, :, None, :]
    v = _share_prompt(_ternary((R, Sk, H, hd), 31), sc)
    for p in range(-(-len(SHARED_PICKS) // R)):
        q = torch.zeros(R, 1, H, hd, dtype=torch.float64)
        for r in range(R):
            q[r, 0, :, :bits] = 32.0 * feat(torch.tensor(shared_target(sc, keep[r, 0, 0], SHARED_PICKS[(r + p * R) % len(SHARED_PICKS)]) + 1))
        yield Probe(f"B[{p}]", q, k, v, None, 1.0, False)


def shared_probes(sc: SharedCase):
    yield from shared_probe_a(sc)
    yield from shared_probe_b(sc)


def shared_buffers(sc: SharedCase, pr: Probe) -> dict:
    """The call's buffers before the step (float64, CPU): qkv [R, 3 E] (q | k_new | v_new), kp / vp [B, S0 + 3, E] with GARBAGE behind
    S0, kt / vt [R, t_max, E] with -GARBAGE in slot t and GARBAGE behind it, mask int32 [B, S0 + 3] or None."""
    B, G, S0, t, H, hd = sc.B, sc.G, sc.S0, sc.n - 1, sc.H, sc.hd
    R, E = B * G, H * hd
    flat = lambda x: x.reshape(*x.shape[:-2], E)
    out = {"qkv": torch.cat([flat(pr.q[:, 0]), flat(pr.k[:, S0 + t]), flat(pr.v[:, S0 + t])], 1), "mask": shared_mask(sc)}
    for name, x in (("k", pr.k), ("v", pr.v)):
        p = torch.full((B, S0 + 3, E), GARBAGE, dtype=torch.float64)
        p[:, :S0] = flat(x[::G, :S0])
        tail = torch.full((R, sc.t_max, E), GARBAGE, dtype=torch.float64)
        tail[:, :t] = flat(x[:, S0:S0 + t])
        tail[:, t] = -GARBAGE
        out[name + "p"], out[name + "t"] = p, tail
    return out


SHARED_MUTATIONS = ("tail_of_next_row", "tail_key_t_dropped", "tail_slot_t+1", "prompt_key_S0", "first_batch_last_key_dropped",
                    "mask_stride_S0", "mask_of_next_prompt", "v_of_head_h^1")


def shared_gather(sc: SharedCase, buf: dict, mutation: Optional[str] = None):
    """(q, k, v, keep) as a kernel reads them out of ``buf``: without a mutation, the probe the buffers were built from; with one, what
    a kernel wrong in that one index sees (a wrongly attended key is appended to its segment of the axis)."""
    B, G, S0, t, H, hd = sc.B, sc.G, sc.S0, sc.n - 1, sc.H, sc.hd
    R, E = B * G, H * hd
    b_of, g_of = torch.arange(R) // G, torch.arange(R) % G
    src = b_of * G + (g_of + 1) % G if mutation == "tail_of_next_row" else torch.arange(R)
    np_ = S0 + (mutation == "prompt_key_S0")
    nt = t + 1 + (mutation == "tail_slot_t+1" and t + 1 < sc.t_max)
    parts = {}
    for i, name in enumerate(("k", "v")):
        new = buf["qkv"][:, (1 + i) * E:(2 + i) * E]
        tail = buf[name + "t"].clone()
        tail[:, t] = new                                                                        # the lanes that own slot t take the new row
        x = torch.cat([buf[name + "p"][b_of, :np_], tail[src, :nt]], 1).reshape(R, np_ + nt, H, hd)
        parts[name] = x
    if mutation == "v_of_head_h^1":
        parts["v"] = parts["v"][:, :, [h ^ 1 if h ^ 1 < H else h for h in range(H)]]
    keep = torch.ones(R, np_ + nt, dtype=torch.bool)
    if buf["mask"] is not None:
        m, ld = buf["mask"].reshape(-1), buf["mask"].shape[1]
        mb = (b_of + 1) % B if mutation == "mask_of_next_prompt" else b_of
        stride = S0 if mutation == "mask_stride_S0" else ld
        keep[:, :np_] = m[(mb * stride)[:, None] + torch.arange(np_)[None]] != 0
    if mutation == "first_batch_last_key_dropped":
        keep[:, min(sc.step, S0) - 1] = False
    if mutation == "tail_key_t_dropped":
        keep[:, np_ + t] = False
    return buf["qkv"][:, :E].reshape(R, 1, H, hd), parts["k"], parts["v"], keep[:, None, None, :]


# =================================================================================================================== merge
# eavqa_attention_merge alone: small integers in o1 / o2 and log-sum-exps that make every weight exactly 0, 0.5 or 1, so that the
# expected output is exact in both storage types and any mix-up of the two lse layouts, of c and t, or of h picks the wrong segment.
MERGE_CASES = [(1, 1, 1, 1, 8), (2, 3, 4, 5, 16), (2, 5, 3, 2, 80), (1, 2, 7, 3, 64), (1, 3, 5, 3, 24)]    # B, C, T, H, hd
MERGE_PATTERNS = ("select", "half", "empty")
LSE_EMPTY = -torch.finfo(torch.float32).max
MERGE_MUTATIONS = ("lse1_as_lse2_layout", "lse2_c_t_swapped", "empty_test_on_wrong_segment")


def merge_inputs(shape, pattern: str):
    """(o1, o2 [B C T, H hd] float64 integers in [-8, 8], lse1 [B, H, C T], lse2 [B C, H, T] float32).  lse1 differs per (b, h, c, t);
    "select": lse2 = lse1 +/- 200 by a fixed pseudo-random sign; "half": lse2 = lse1; "empty": a quarter each of lse1, lse2, both,
    neither (= "select") at an empty value (-FLT_MAX in lse2, -0.3 FLT_MAX in lse1)."""
    B, C, T, H, hd = shape
    g = torch.Generator().manual_seed(50 + B * C * T * H + hd)
    o1, o2 = (torch.randint(-8, 9, (B * C * T, H * hd), generator=g).double() for _ in range(2))
    lse1 = (0.25 * torch.randperm(B * H * C * T, generator=g).float() - 3.0).reshape(B, H, C * T)
    l1 = lse1.reshape(B, H, C, T).permute(0, 2, 1, 3)                                          # [B, C, H, T]
    sign = (torch.randint(0, 2, (B, C, H, T), generator=g) * 2 - 1).float()
    lse2 = l1 + (0.0 if pattern == "half" else 200.0) * sign
    if pattern == "empty":
        kind = torch.randint(0, 4, (B, C, H, T), generator=g)
        kind.reshape(-1)[:4] = torch.arange(4)[:kind.numel()]                                   # every kind, whenever there is room
        lse2 = torch.where(kind >= 2, torch.full_like(lse2, LSE_EMPTY), lse2)
        l1 = torch.where(kind % 2 == 1, torch.full_like(l1, 0.3 * LSE_EMPTY), l1)                # just below the -0.25 FLT_MAX threshold
        lse1 = l1.permute(0, 2, 1, 3).reshape(B, H, C * T)
    return o1, o2, lse1.contiguous(), lse2.reshape(B * C, H, T).contiguous()


def merge_emulate(shape, o1, o2, lse1, lse2, mutation: Optional[str] = None):
    """The merge as csrc/score.hip states it, float32 weights, one element at a time from the flat lse buffers - or wrong in one index."""
    B, C, T, H, hd = shape
    row = torch.arange(B * C * T)
    t, bc = row % T, row // T
    b, c = bc // C, bc % C
    h = torch.arange(H)[None, :]
    b, c, t, bc = b[:, None], c[:, None], t[:, None], bc[:, None]
    i1 = (b * H + h) * (C * T) + c * T + t
    i2 = (bc * H + h) * T + t
    if mutation == "lse1_as_lse2_layout":
        i1 = i2
    if mutation == "lse2_c_t_swapped":                                                          # the row decoded t-major
        ct = c * T + t
        i2 = ((b * C + ct % C) * H + h) * T + ct // C
    l1, l2 = lse1.reshape(-1)[i1], lse2.reshape(-1)[i2]                                         # [rows, H] float32
    e1, e2 = l1 < 0.25 * LSE_EMPTY, l2 < 0.25 * LSE_EMPTY
    m = torch.maximum(l1, l2)
    w1, w2 = torch.exp(l1 - m), torch.exp(l2 - m)
    inv = 1.0 / (w1 + w2)
    w1, w2 = (w1 * inv).double(), (w2 * inv).double()
    if mutation == "empty_test_on_wrong_segment":
        w1, w2 = torch.where(e1, 1.0, torch.where(e2, 0.0, w1)), torch.where(e1, 0.0, torch.where(e2, 1.0, w2))
    else:
        w1, w2 = torch.where(e1, 0.0, torch.where(e2, 1.0, w1)), torch.where(e1, 1.0, torch.where(e2, 0.0, w2))
    wide = lambda w: w.repeat_interleave(hd, 1)
    return wide(w1) * o1 + wide(w2) * o2


def merge_expected(shape, o1, o2, lse1, lse2):
    """What the merge must return, from the construction alone: o2 where lse1 is empty, else o1 where lse2 is empty or 200 below, o2
    where it is 200 above, their mean where the two are equal."""
    B, C, T, H, hd = shape
    l1 = lse1.reshape(B, H, C, T).permute(0, 2, 3, 1).reshape(B * C * T, H).double()
    l2 = lse2.reshape(B, C, H, T).permute(0, 1, 3, 2).reshape(B * C * T, H).double()
    w2 = torch.where(l1 < 0.25 * LSE_EMPTY, 1.0, torch.where(l2 < 0.25 * LSE_EMPTY, 0.0, torch.where(l2 > l1, 1.0, torch.where(l2 < l1, 0.0, 0.5))))
    w2 = w2.repeat_interleave(hd, 1)
    return (1.0 - w2) * o1 + w2 * o2


# =================================================================================================================== score flow
# attention_fwd over the shared prompt (B, C T query rows, key mask), attention_fwd over each candidate's own tokens (B C, causal) and
# attention_merge, against ONE attention over [masked prompt | candidate's causal prefix]: an ordinary causal case of B C samples with
# Sq = T and Sk = S0 + T (query i sits at position S0 + i).
@dataclass(frozen=True)
class FlowCase:
    B: int
    C: int
    T: int
    S0: int
    hd: int
    dtype: str
    masked_prompt: Optional[int] = None         # this prompt has every key masked
    H: int = 2

    @property
    def case(self) -> Case:
        return Case(self.B * self.C, self.H, self.T, self.S0 + self.T, self.hd, True, "flow")

    @property
    def torch_dtype(self):
        return torch.bfloat16 if self.dtype == "bf16" else torch.float32

    @property
    def id(self):
        return f"{self.dtype}-{self.B}x{self.C}x{self.T}-S{self.S0}-hd{self.hd}" + ("" if self.masked_prompt is None else f"-prompt{self.masked_prompt}masked")


SCORE_FLOW_CASES = [FlowCase(2, 3, 5, 65, 64, "bf16"), FlowCase(1, 2, 17, 129, 80, "bf16"), FlowCase(2, 1, 1, 1, 64, "bf16"),
                    FlowCase(2, 3, 5, 37, 16, "fp32"), FlowCase(2, 3, 5, 65, 64, "bf16", masked_prompt=1)]


def flow_mask(fc: FlowCase) -> torch.Tensor:
    """int32 [B, S0]: holes (the last prompt key visible), or nothing at all for ``masked_prompt``."""
    g = torch.Generator().manual_seed(3000 + 7 * fc.S0 + fc.hd)
    m = (torch.rand(fc.B, fc.S0, generator=g) > 0.3).int()
    m[:, fc.S0 - 1] = 1
    if fc.masked_prompt is not None:
        m[fc.masked_prompt] = 0
    return m


def flow_keep(fc: FlowCase) -> torch.Tensor:
    km = torch.cat([flow_mask(fc).repeat_interleave(fc.C, 0), torch.ones(fc.B * fc.C, fc.T, dtype=torch.int32)], 1)
    return visible(fc.case, km)


FLOW_PICKS = ("diagonal", "first candidate", "last prompt", "first prompt", "middle")


def flow_target(fc: FlowCase, i: int, vis, pick: str) -> int:
    prompt = [j for j in vis if j < fc.S0]
    if pick == "diagonal" or (not prompt and pick != "first candidate"):
        return fc.S0 + i
    return {"first candidate": fc.S0, "last prompt": prompt[-1] if prompt else 0, "first prompt": prompt[0] if prompt else 0,
            "middle": vis[len(vis) // 2]}[pick]


def flow_probes(fc: FlowCase):
    """Probe A with (1 + h) in the prompt and (1 + h)(1 + c) in candidate c's own keys; Probe B one-hot, row (bc, i) of probe p asking
    for pick (bc + i + p) mod 5.  The prompt part of K and V is the same for the C candidates of a question."""
    case, keep = fc.case, flow_keep(fc)
    N, H, T, Sk, hd = case.B, case.H, case.Sq, case.Sk, case.hd

    def share(x):
        x[:, :fc.S0] = x[::fc.C, :fc.S0].repeat_interleave(fc.C, 0)
        return x

    factor = torch.ones(N, Sk, 1, 1, dtype=torch.float64)
    factor[:, fc.S0:] *= (1.0 + (torch.arange(N) % fc.C).double())[:, None, None, None]
    for pr in probe_a_forward(case):
        yield pr._replace(k=share(pr.k.clone()), v=pr.v * factor)
    ok = torch.ones(N, T, dtype=torch.bool)
    for p in range(len(FLOW_PICKS)):
        pick = lambda b, i, vis: flow_target(fc, i, vis, FLOW_PICKS[(b + i + p) % len(FLOW_PICKS)])
        pr = probe_b(case, keep, ok, backward=False, target=pick)
        yield pr._replace(name=f"B[{p}]", v=share(pr.v.clone()))


def flow_emulate(fc: FlowCase, pr: Probe, keep: torch.Tensor, rnd=None):
    """The two segments and their merge in float64, ``rnd`` applied to o1, o2 and the merged output: [B C, T, H, hd]."""
    rnd = rnd or (lambda x: x)
    S0 = fc.S0
    s1 = reference(pr.q, pr.k[:, :S0], pr.v[:, :S0], None, keep[..., :S0], None, pr.scale)
    s2 = reference(pr.q, pr.k[:, S0:], pr.v[:, S0:], None, keep[..., S0:], None, pr.scale)
    some1 = keep[..., :S0].any(-1).expand(-1, fc.H, -1)                                         # [N, H, T]
    l1 = torch.where(some1, s1.lse, torch.full_like(s1.lse, -math.inf))
    m = torch.maximum(l1, s2.lse)
    w1, w2 = torch.exp(l1 - m), torch.exp(s2.lse - m)
    w = lambda x: (x / (w1 + w2)).permute(0, 2, 1)[..., None]
    return rnd(w(w1) * rnd(s1.val["o"]) + w(w2) * rnd(s2.val["o"]))
