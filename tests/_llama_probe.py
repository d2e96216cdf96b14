"""Exact and bounded probes of the Llama-family kernels (csrc/llama.hip): eavqa_rope, eavqa_rope_finish, eavqa_swiglu_fwd / _bwd / _splitk -
case tables, plain float64 references, acceptance functions and CPU emulations with one-line mutations (no GPU needed here).

Conventions of tests/_gemm_probe.py: every matrix of a call is a window into a flat buffer.  Input pads hold NaN; output pads and one guard
row before and after hold SENTINEL, and `untouched` tells whether a kernel wrote one of them (x of eavqa_rope is rotated in place: it is
an output, its pads hold the sentinel, which is finite and far outside every value a case can produce).

Rope: exact by construction.  eavqa_rope takes ANY table, so the probe supplies its own (models/lm.py's rope_table is not used): cos[p, i]
and sin[p, i] are multiples of 1/4 in [-1, 1], x holds integers with |v| <= 8.  A product a c is then a multiple of 1/4 of magnitude <= 8
and the two-term sum a c -+ b s a multiple of 1/4 of magnitude <= 16: at most 7 significant bits, exact in float32 and in bfloat16 (8 bits)
whether the compiler contracts the sum to an FMA or not.  The expectation is therefore EQUALITY with the float64 reference, element by
element.  eavqa_rope_finish sums ks <= 4 slices of integers with |v| <= 2 first (|sum| <= 8, exact in any order), so the same holds;
tests/test_llama_probe_cpu.py asserts that every expected value of every case survives a round trip through bfloat16.

SwiGLU: a per-element bound.  The kernels compute s = rcp(1 + __expf(-g)) in float32 (fast_sigmoid of csrc/common.h), silu = g s and
silu' = s (1 + g (1 - s)).  The error of s has three parts: the float32 rounding of -g log2(e), which feeds the hardware exp2 and is an
ABSOLUTE error of about |g| log2(e) 2^-24 in the exponent, that is a relative error of about |g| 2^-24 of the result - it grows with |g| -
and the instruction accuracies of exp2 and rcp.  Neither the kernel guides nor any document shipped with the toolchain states those two
accuracies, so they were MEASURED, once, on an MI355X: 14.7 M float32 gates (linear, uniform and normal in [-32, 32] plus 2 M gates of
magnitude 2^-40 .. 2^5) through eavqa_swiglu_fwd / _bwd with up = dh = 1, against float64.  Worst observed relative error: silu
1.8576e-6, silu' 1.7483e-6 (relative to s (1 + |g| (1 - s)), the sum of the magnitudes of its terms - the value itself passes through
zero at g = -1.2785); both grow with |g| as the argument above says (5.5e-7 below |g| = 8, 1.0e-6 below 16, 1.8e-6 below 32; 3.9e-6 at
|g| = 87).  The constants are FOUR times the worst observation, the margin covering gates the sweep did not hit:

    C_SILU = 4 * 1.8576e-6 = 7.43e-6        C_DSILU = 4 * 1.7483e-6 = 6.99e-6        for |g| <= G_TABLED = 32.

Propagation, with u = 2^-24 (float32) / 2^-8 (bfloat16: 8 significant bits, round to nearest) the rounding of the stored type:
    fwd, splitk   ref = silu(g) b        e = |ref| (C_SILU + 2^-24)                  (one more float32 product)
    bwd, du[:, F:] ref = dh silu(g)      e = |ref| (C_SILU + 2^-24)
    bwd, du[:, :F] ref = dh b silu'(g)   e = |dh b| s (1 + |g| (1 - s)) (C_DSILU + 2^-23)   (two more products)
    bound = e + u (|ref| + e) + floor,   floor = 2^-126 (1 + min(|g|, 128)) max(1, |multiplier|):
the floor is for results below the float32 normal range, which the hardware may flush - for g <= -87 the kernel may return +-0 where the
reference is a tiny normal number.  Beyond the tabled range (the edge table: |g| = 87, 89, 104 and the largest finite value, where
__expf overflows and the reciprocal returns 0) three things are asserted instead: the output is finite; for g > 0, where s is 1 in
float32 from g = 17 on, it equals g b (dh b, dh g) to one rounding: relative u, plus 2^-24 for bfloat16, whose rounding follows the
float32 product's, plus (1 + g) e^-g for the distance of the function itself from the line; for g < 0 its magnitude is no larger than
|ref| (1 + u + C |g| / 32) + floor - the measured constant scaled with |g| as its dominant term scales.  No infinities: torch's own
silu(-inf) is NaN.  All inputs are exact in bfloat16 (the edge gates: rounded to the case's type), so the float64 reference sees the
values the kernel sees.

The references are loops over rows / tensor expressions in float64 and share no code with tests/_llama_ref.py, ops or the emulations
below, which walk the data as the kernels do - items of VEC columns, grid-stride passes of 524 288 items, slices in order - and take
the one-line mutations of MUTATIONS, each of which tests/test_llama_probe_cpu.py requires a named case to reject.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from _gemm_probe import NAN, SENTINEL, on_device, untouched, window  # noqa: F401

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
U = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8}
BLOCK = 256
MAX_BLOCKS = 256 * 8
PASS = BLOCK * MAX_BLOCKS                   # 524 288 items: what one grid-stride pass of rope / swiglu_fwd / swiglu_bwd covers
N_POS = 13
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

C_SILU = 4 * 1.8576e-6                      # measured, see the module docstring
C_DSILU = 4 * 1.7483e-6
G_TABLED = 32.0
FLOOR = 2.0 ** -126
SILU_GRAD_ZERO = 1.2784645427610738         # silu'(-z) = 0

WORST = {}                                  # (entry point, type) -> worst error / bound seen by check_swiglu


def _idx(n):
    return torch.arange(n, dtype=torch.int64)


def _first(got, want):
    bad = (got != want) | got.isnan()
    if not bad.any():
        return "none"
    r, c = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} elements differ, first at (row {r}, column {c}): got {got[r, c].item()}, want {want[r, c].item()}"


def _round(v, dtype: str):
    return v.to(DT[dtype]).double()


# ==================================================================================================================== tables, positions
def table_values(n_pos: int, cols: int):
    """(cos, sin) float64 [n_pos, cols]: multiples of 1/4 in [-1, 1], different steps along the two axes, the two tables different."""
    p, i = _idx(n_pos)[:, None], _idx(cols)[None, :]
    return ((3 * p + 5 * i + 1) % 9 - 4).double() / 4, ((5 * p + 2 * i + 3) % 9 - 4).double() / 4


def positions(rows: int, kind: str):
    """int32 [rows].  mixed: packed restarts (non-monotonic, repeated), row 0 at n_pos - 1, row 1 at 0, rows 2, 3, 5, 6 out of range on both
    sides, and further out-of-range rows every 97 (a skipped row in every pass of a multi-pass case); last / zero / below / above: every
    row there."""
    if kind != "mixed":
        return torch.full((rows,), {"last": N_POS - 1, "zero": 0, "below": -1, "above": N_POS}[kind], dtype=torch.int32)
    r = _idx(rows)
    p = (r % 5) * 2 + (r // 5) % 3
    p = torch.where(r % 97 == 50, -1 - r % 3, p)
    p = torch.where(r % 97 == 51, N_POS + r % 5, p)
    for row, v in ((0, N_POS - 1), (1, 0), (2, -1), (3, N_POS), (4, 9), (5, INT_MIN), (6, INT_MAX), (7, 9)):
        if row < rows:
            p[row] = v
    return p.to(torch.int32)


def _table_windows(table_cols: int, ld_table: int):
    cos, sin = table_values(N_POS, table_cols)
    out = {}
    for nm, t in (("cos", cos), ("sin", sin)):
        bk, vw = window(N_POS, table_cols, ld_table, torch.float32, fill=NAN)
        vw.copy_(t)
        out[nm] = (bk, vw)
    return out, cos, sin


def _table_geometry(i: int, hd: int):
    """(table_cols, ld_table) of variant i: contiguous; four pad columns; a table built for a head of 2 hd columns."""
    half = hd // 2
    return [(half, half), (half, half + 4), (hd, hd)][i % 3]


# =============================================================================================================================== rope
@dataclass(frozen=True)
class RopeCase:
    name: str
    dtype: str
    hd: int
    H: int
    rows: int
    ldx: int
    table_cols: int
    ld_table: int
    inverse: bool
    pos_kind: str = "mixed"
    multipass: bool = False

    @property
    def vec(self):
        return 8 if self.dtype == "bf16" and self.hd % 16 == 0 else 4

    @property
    def per_head(self):
        return self.hd // 2 // self.vec

    @property
    def per_row(self):
        return self.H * self.per_head

    @property
    def items(self):
        return self.rows * self.per_row

    @property
    def route(self):
        return f"{self.dtype}-vec{self.vec}"


ROPE_HD = {"f32": (8, 24, 64), "bf16": (16, 32, 128, 8, 24, 40)}


def _build_rope_cases():
    cases, i = [], 0
    for dtype, hds in ROPE_HD.items():
        for hd in hds:
            for H in (1, 3, 6):
                for rows in (1, 5, 67):
                    tc, ldt = _table_geometry(i + i // 3, hd)
                    kind = "mixed" if rows > 1 else ("last", "zero", "below", "above")[(i // 3) % 4]
                    inv = (i + i // 9) % 2 == 1
                    cases.append(RopeCase(f"rope-{dtype}-hd{hd}-H{H}-r{rows}-ldt{ldt}-{'inv' if inv else 'fwd'}-{kind}", dtype, hd, H, rows,
                                          H * hd + (8, 16)[i % 2], tc, ldt, inv, kind))
                    i += 1
    # three grid-stride passes per instantiation: small heads, many of them (the properties are asserted by multipass_violations)
    cases.append(RopeCase("rope-multipass-f32-vec4", "f32", 8, 511, 2053, 511 * 8 + 4, 4, 8, False, "mixed", True))
    cases.append(RopeCase("rope-multipass-bf16-vec8", "bf16", 16, 511, 2053, 511 * 16 + 8, 16, 16, True, "mixed", True))
    cases.append(RopeCase("rope-multipass-bf16-vec4-per_head3", "bf16", 24, 170, 2057, 170 * 24 + 8, 12, 16, False, "mixed", True))
    return cases


def multipass_violations(items: int, per_row: int):
    """What keeps a case from being a three-pass case with a ragged tail whose pass boundaries fall inside rows (empty: nothing)."""
    bad = []
    if not 2 * PASS < items <= 3 * PASS:
        bad.append(f"{items} items are not three passes of {PASS}")
    if items % BLOCK == 0:
        bad.append("the item count is a multiple of the block")
    for k in (1, 2):
        if (k * PASS) % per_row == 0:
            bad.append(f"pass boundary {k} falls on a row boundary")
    return bad


def x_values(rows: int, cols: int):
    r, c = _idx(rows)[:, None], _idx(cols)[None, :]
    return ((3 * r + 5 * c + 1) % 17 - 8).double()


def materialize_rope(c: RopeCase):
    """(windows, values): x (the sentinel around it, one guard row before and after), the two tables (NaN pads), pos."""
    win, cos, sin = _table_windows(c.table_cols, c.ld_table)
    x = x_values(c.rows, c.H * c.hd)
    bk, vw = window(c.rows, c.H * c.hd, c.ldx, DT[c.dtype], elem_offset=c.ldx, fill=SENTINEL)
    vw.copy_(x)
    win["x"] = (bk, vw)
    pos = positions(c.rows, c.pos_kind)
    return win, {"x": x, "cos": cos, "sin": sin, "pos": pos}


def _rotate_row(v, cr, sr):
    """v [heads, hd] float64 -> rotate_half convention, cr / sr [hd / 2]."""
    half = v.shape[1] // 2
    a, b = v[:, :half], v[:, half:]
    return torch.cat([a * cr - b * sr, b * cr + a * sr], dim=1)


def reference_rope(c: RopeCase, v: dict):
    want = v["x"].clone()
    half = c.hd // 2
    for r in range(c.rows):
        p = int(v["pos"][r])
        if not 0 <= p < N_POS:
            continue
        sr = v["sin"][p, :half]
        want[r] = _rotate_row(v["x"][r].view(c.H, c.hd), v["cos"][p, :half], -sr if c.inverse else sr).reshape(-1)
    return want


def check_rope(c, want, backing, view, what="x"):
    """Raises AssertionError unless the window holds exactly `want` and nothing outside it was written."""
    assert untouched(backing, view), f"{c.name}: {what} was written outside its window (pad column or guard row)"
    got = view.double()
    assert torch.equal(got, want), f"{c.name}: {what} differs from the exact rotation: {_first(got, want)}"


def _passes(n: int, mutation: Optional[str]):
    """The items of every grid-stride pass of a launch of min(ceil(n / 256), 2048) blocks."""
    T = min(-(-n // BLOCK), MAX_BLOCKS) * BLOCK
    stride = T
    if mutation == "stride_short_one_block" and T > BLOCK:
        stride = T - BLOCK
    if mutation == "last_partial_block_dropped":
        n = n // BLOCK * BLOCK
    k = 0
    while k * stride < n:
        idx = k * stride + _idx(T)
        yield idx[idx < n]
        if mutation == "later_passes_skipped":
            return
        k += 1


def _take(flat, idx):
    return flat[idx.clamp(0, flat.numel() - 1)]


def _put(flat, idx, vals):
    """A store by element index; an index outside the buffer lands on its first / last element, which is a guard: `untouched` sees it."""
    flat[idx.clamp(0, flat.numel() - 1)] = vals


def _table_reads(mutation, p, r, j, half, ldt, cosf, sinf):
    """cos / sin [items, VEC] as the kernels address them: table + p ld_table + column."""
    if mutation == "table_row_is_r":
        p = r
    stride = half if mutation == "table_stride_half" else ldt
    col = j + (half if mutation == "table_col_plus_half" else 0)
    ti = p[:, None] * stride + col
    return _take(cosf, ti), _take(sinf, ti)


ROPE_MUTATIONS = ("interleaved_pairs", "sin_sign", "inverse_ignored", "table_stride_half", "table_col_plus_half", "table_row_is_r",
                  "clamp_position", "later_passes_skipped", "stride_short_one_block", "last_partial_block_dropped", "vec4_ignores_per_head")


def emulate_rope(c: RopeCase, win: dict, v: dict, mutation: Optional[str] = None):
    """rope_kernel<T, VEC> in index arithmetic over the flat buffers, in place in win["x"]."""
    bk, vw = win["x"]
    X = bk.double()
    off, ldx = vw.storage_offset(), vw.stride(0)
    cosf, sinf = win["cos"][0].double(), win["sin"][0].double()
    pos = v["pos"].long()
    half, VEC, per_head, per_row = c.hd // 2, c.vec, c.per_head, c.per_row
    for idx in _passes(c.items, mutation):
        r = idx // per_row
        rem = idx - r * per_row
        h = rem // per_head
        i = (rem - h * per_head) * VEC
        if mutation == "vec4_ignores_per_head" and c.route == "bf16-vec4":
            i = torch.zeros_like(i)
        p = pos[r]
        ok = (p >= 0) & (p < N_POS)
        if mutation == "clamp_position":
            p, ok = p.clamp(0, N_POS - 1), torch.ones_like(ok)
        r, h, i, p = r[ok], h[ok], i[ok], p[ok]
        j = i[:, None] + _idx(VEC)[None, :]
        base = (off + r * ldx + h * c.hd)[:, None]
        lo, hi = base + j, base + j + half
        if mutation == "interleaved_pairs":
            lo, hi = base + 2 * j, base + 2 * j + 1
        cc, ss = _table_reads(mutation, p, r, j, half, c.ld_table, cosf, sinf)
        if c.inverse and mutation != "inverse_ignored":
            ss = -ss
        if mutation == "sin_sign":
            ss = -ss
        a, b = X[lo], X[hi]
        _put(X, lo, _round(a * cc - b * ss, c.dtype))
        _put(X, hi, _round(b * cc + a * ss, c.dtype))
    bk.copy_(X)


# ======================================================================================================================== rope_finish
@dataclass(frozen=True)
class FinishCase:
    name: str
    out: str
    ks: int
    M: int
    H: int
    hd: int
    ld_out: int
    table_cols: int
    ld_table: int
    pos_kind: str

    @property
    def E(self):
        return self.H * self.hd


def _build_finish_cases():
    cases, i = [], 0
    for H, hd in ((3, 8), (2, 24), (2, 64), (1, 128)):
        for ks in (1, 3, 4):
            for M in (1, 33, 64):
                for out in ("f32", "bf16"):
                    tc, ldt = _table_geometry(i + 1 + i // 6, hd)               # ld_table > hd / 2 in two of three
                    kind = "mixed" if M > 1 else ("last", "above", "zero")[(i // 6 + i % 2) % 3]
                    ld_out = 3 * H * hd + 4 * (1 + i % 3)
                    cases.append(FinishCase(f"finish-{out}-H{H}-hd{hd}-ks{ks}-M{M}-ldo{ld_out}-ldt{ldt}-{kind}", out, ks, M, H, hd, ld_out, tc, ldt, kind))
                    i += 1
    return cases


def partial_values(ks: int, M: int, cols: int, lim: int = 2, scale: float = 1.0):
    """[ks, M, cols] float64: slice s holds its own pattern of integers in [-lim, lim] (times scale) - a skipped, repeated or misplaced
    slice changes the sum."""
    r, c = _idx(M)[:, None], _idx(cols)[None, :]
    return torch.stack([(((3 + 2 * s) * r + (5 + s) * c + 7 * s) % (2 * lim + 1) - lim).double() * scale for s in range(ks)])


def _out_offset(ld: int) -> int:
    return (ld + 7) // 8 * 8                     # one guard row before the output, the base still 16-byte aligned in bfloat16


def materialize_finish(c: FinishCase):
    win, cos, sin = _table_windows(c.table_cols, c.ld_table)
    part = partial_values(c.ks, c.M, 3 * c.E)
    bk, vw = window(c.ks * c.M, 3 * c.E, 3 * c.E, torch.float32, fill=NAN)
    vw.copy_(part.view(c.ks * c.M, 3 * c.E))
    win["part"] = (bk, vw)
    win["out"] = window(c.M, 3 * c.E, c.ld_out, DT[c.out], elem_offset=_out_offset(c.ld_out), fill=SENTINEL)
    return win, {"part": part, "cos": cos, "sin": sin, "pos": positions(c.M, c.pos_kind)}


def reference_finish(c: FinishCase, v: dict):
    """Rows summed over the slices; q and k (the first 2 H heads) rotated where pos is in range; v the plain sum."""
    acc = torch.zeros(c.M, 3 * c.E, dtype=torch.float64)
    for s in range(c.ks):
        acc += v["part"][s]
    want = acc.clone()
    half = c.hd // 2
    for m in range(c.M):
        p = int(v["pos"][m])
        if 0 <= p < N_POS:
            want[m, :2 * c.E] = _rotate_row(acc[m, :2 * c.E].view(2 * c.H, c.hd), v["cos"][p, :half], v["sin"][p, :half]).reshape(-1)
    return want


FINISH_MUTATIONS = ("v_rotated", "slice_skipped", "slice_stride_3E", "ld_out_ignored", "table_stride_half", "table_col_plus_half", "table_row_is_r",
                    "clamp_position", "sin_sign", "interleaved_pairs")


def emulate_finish(c: FinishCase, win: dict, v: dict, mutation: Optional[str] = None):
    """rope_finish_kernel: one item per thread, 2 H (hd / 8) rotated items then E / 4 plain ones per row."""
    P = win["part"][0].double()
    cosf, sinf = win["cos"][0].double(), win["sin"][0].double()
    ob, ov = win["out"]
    O = ob.double()
    off, ldo = ov.storage_offset(), (3 * c.E if mutation == "ld_out_ignored" else ov.stride(0))
    E, half = c.E, c.hd // 2
    per_head = half // 4
    n_rot = (3 if mutation == "v_rotated" else 2) * c.H * per_head
    per_row = n_rot + (0 if mutation == "v_rotated" else E // 4)
    N3 = 3 * E
    slice_ = N3 if mutation == "slice_stride_3E" else c.M * N3
    pos = v["pos"].long()
    q = _idx(4)[None, :]

    def sums(m, col):
        acc = torch.zeros(col.shape, dtype=torch.float64)
        for s in range(c.ks):
            if mutation == "slice_skipped" and s == 1:
                continue
            acc = acc + _take(P, s * slice_ + (m * N3)[:, None] + col)
        return acc

    idx = _idx(c.M * per_row)
    m, it = idx // per_row, idx % per_row
    plain = it >= n_rot
    mp, col = m[plain], (2 * E + (it[plain] - n_rot) * 4)[:, None] + q
    _put(O, off + (mp * ldo)[:, None] + col, _round(sums(mp, col), c.out))
    m, it = m[~plain], it[~plain]
    h = it // per_head
    i = (it - h * per_head) * 4
    j = i[:, None] + q
    lo = (h * c.hd)[:, None] + j
    hi = lo + half
    if mutation == "interleaved_pairs":
        lo = (h * c.hd)[:, None] + 2 * j
        hi = lo + 1
    a, b = sums(m, lo), sums(m, hi)
    p = pos[m]
    ok = (p >= 0) & (p < N_POS)
    if mutation == "clamp_position":
        p, ok = p.clamp(0, N_POS - 1), torch.ones_like(ok)
    cc, ss = _table_reads(mutation, p, m, j, half, c.ld_table, cosf, sinf)          # (an out-of-range row reads a clamped index and keeps a, b)
    if mutation == "sin_sign":
        ss = -ss
    okc = ok[:, None]
    ra = torch.where(okc, a * cc - b * ss, a)
    rb = torch.where(okc, b * cc + a * ss, b)
    _put(O, off + (m * ldo)[:, None] + lo, _round(ra, c.out))
    _put(O, off + (m * ldo)[:, None] + hi, _round(rb, c.out))
    ob.copy_(O)


# ============================================================================================================================= SwiGLU
@dataclass(frozen=True)
class SwigluCase:
    name: str
    kind: str                       # fwd | bwd | splitk
    dtype: str                      # fwd / bwd: of every operand; splitk: of the output
    rows: int
    F: int
    ldu: int = 0                    # fwd / bwd
    ldh: int = 0                    # fwd: h; bwd: dh; splitk: out
    lddu: int = 0                   # bwd
    ks: int = 0                     # splitk
    edge: bool = False
    multipass: bool = False

    @property
    def items(self):
        return self.rows * (self.F // 4)


def edge_gates(dtype: str):
    """+-0, the zero of silu' (rounded to the type), +-16 (s rounds to 1 from 17 on), +-30, and beyond the tabled range +-87 (the last
    gate whose exp is finite), +-89 (exp overflows), +-104, +- the largest finite value."""
    big = torch.finfo(DT[dtype]).max
    g = torch.tensor([0.0, -0.0, SILU_GRAD_ZERO, -SILU_GRAD_ZERO, 16.0, -16.0, 30.0, -30.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, big, -big],
                     dtype=torch.float64)
    return _round(g, dtype)


def _build_swiglu_cases():
    cases, i = [], 0
    for kind in ("fwd", "bwd", "splitk"):
        for dtype in ("f32", "bf16"):
            for F in (4, 32, 160, 2052):
                for rows in (1, 5, 65):
                    if kind == "splitk":
                        ks = (1, 3, 4)[i % 3]
                        cases.append(SwigluCase(f"swiglu-splitk-{dtype}-F{F}-r{rows}-ks{ks}", kind, dtype, rows, F, ldh=F + 4 * (1 + i % 2), ks=ks))
                    else:
                        cases.append(SwigluCase(f"swiglu-{kind}-{dtype}-F{F}-r{rows}", kind, dtype, rows, F, ldu=2 * F + 8, ldh=F + (4, 12)[kind == "bwd"],
                                                lddu=2 * F + 4 if kind == "bwd" else 0))
                    i += 1
            n_edge = edge_gates(dtype).numel()
            if kind == "splitk":
                cases.append(SwigluCase(f"swiglu-splitk-{dtype}-edge", kind, dtype, 4, n_edge, ldh=n_edge + 4, ks=2, edge=True))
            else:
                cases.append(SwigluCase(f"swiglu-{kind}-{dtype}-edge", kind, dtype, 4, n_edge, ldu=2 * n_edge + 8, ldh=n_edge + (4, 12)[kind == "bwd"],
                                        lddu=2 * n_edge + 4 if kind == "bwd" else 0, edge=True))
    for kind in ("fwd", "bwd"):
        for dtype in ("f32", "bf16"):
            cases.append(SwigluCase(f"swiglu-multipass-{kind}-{dtype}", kind, dtype, 1027, 4100, ldu=8200 + 8, ldh=4100 + (4, 12)[kind == "bwd"],
                                    lddu=8200 + 4 if kind == "bwd" else 0, multipass=True))
    return cases


def swiglu_values(c: SwigluCase):
    """(g, b, d) float64 [rows, F], exact in bfloat16: gates in [-30, 30] in steps of 1/4, up in [-2, 2] and dh in [-1, 1] in steps of 1/8,
    each its own function of (row, column); the edge cases: one gate per column, |up|, |dh| <= 1 so that nothing overflows."""
    r, col = _idx(c.rows)[:, None], _idx(c.F)[None, :]
    if c.edge:
        g = edge_gates(c.dtype)[None, :].expand(c.rows, c.F).clone()
        b = torch.tensor([1.0, -0.5, 0.25, -1.0], dtype=torch.float64)[(r + col) % 4]
        d = torch.tensor([0.5, 1.0, -1.0, -0.25], dtype=torch.float64)[(3 * r + col) % 4]
        return g, b, d
    g = ((7 * r + 3 * col + 5) % 241 - 120).double() / 4
    b = ((5 * r + 3 * col + 1) % 33 - 16).double() / 8
    d = ((3 * r + 7 * col + 2) % 17 - 8).double() / 8
    return g, b, d


def materialize_swiglu(c: SwigluCase):
    g, b, d = swiglu_values(c)
    win = {}
    if c.kind == "splitk":
        u = torch.cat([g, b], dim=1)
        if c.edge:
            part = torch.stack([torch.zeros_like(u), u])                                # (no sum of an edge gate with anything is exact)
        else:
            rest = partial_values(c.ks, c.rows, 2 * c.F, lim=4, scale=0.25)[1:]        # multiples of 1/8 below 64: every order of the sum is exact
            part = torch.cat([(u - rest.sum(0))[None], rest])
        bk, vw = window(c.ks * c.rows, 2 * c.F, 2 * c.F, torch.float32, fill=NAN)
        vw.copy_(part.view(c.ks * c.rows, 2 * c.F))
        win["part"] = (bk, vw)
        win["out"] = window(c.rows, c.F, c.ldh, DT[c.dtype], elem_offset=c.ldh, fill=SENTINEL)
        return win, {"g": g, "b": b, "d": d, "part": part}
    bk, vw = window(c.rows, 2 * c.F, c.ldu, DT[c.dtype], fill=NAN)
    vw.copy_(torch.cat([g, b], dim=1))
    win["u"] = (bk, vw)
    if c.kind == "fwd":
        win["out"] = window(c.rows, c.F, c.ldh, DT[c.dtype], elem_offset=c.ldh, fill=SENTINEL)
    else:
        bk, vw = window(c.rows, c.F, c.ldh, DT[c.dtype], fill=NAN)
        vw.copy_(d)
        win["dh"] = (bk, vw)
        win["out"] = window(c.rows, 2 * c.F, c.lddu, DT[c.dtype], elem_offset=c.lddu, fill=SENTINEL)
    return win, {"g": g, "b": b, "d": d}


def reference_swiglu(c: SwigluCase, v: dict):
    """float64: {"out": the result, "lin": what it tends to for large g, "mag": the magnitude the relative error constant applies to,
    "mult": the multiplier of silu / silu', "g": the gate of every output column}."""
    g, b, d = v["g"], v["b"], v["d"]
    s, t = torch.sigmoid(g), torch.sigmoid(-g)                     # t = 1 - s without the cancellation
    silu, dsilu, dmag = g * s, s * (1 + g * t), s * (1 + g.abs() * t)
    if c.kind != "bwd":
        return {"out": silu * b, "lin": g * b, "mag": (silu * b).abs(), "mult": b, "g": g, "const": torch.full_like(g, C_SILU + 2.0 ** -24)}
    cat = lambda x, y: torch.cat([x, y], dim=1)
    return {"out": cat(d * b * dsilu, d * silu), "lin": cat(d * b, d * g), "mag": cat((d * b).abs() * dmag, (d * silu).abs()), "mult": cat(d * b, d),
            "g": cat(g, g), "const": cat(torch.full_like(g, C_DSILU + 2.0 ** -23), torch.full_like(g, C_SILU + 2.0 ** -24))}


def check_swiglu(c: SwigluCase, ref: dict, backing, view):
    """Raises AssertionError unless every element is inside the bound of the module docstring and nothing outside the window was written."""
    entry = f"eavqa_swiglu_{c.kind}"
    assert untouched(backing, view), f"{c.name}: {entry} wrote outside its window (pad column or guard row)"
    got = view.double()
    want, g, u = ref["out"], ref["g"], U[c.dtype]
    assert bool(got.isfinite().all()), f"{c.name}: non-finite output: {_first(got, want)}"
    floor = FLOOR * (1 + g.abs().clamp_max(128.0)) * ref["mult"].abs().clamp_min(1.0)
    err = (got - want).abs()
    e = ref["mag"] * ref["const"]
    bound = e + u * (want.abs() + e) + floor
    inside = g.abs() <= G_TABLED
    ratio = torch.where(inside, err / bound, torch.zeros_like(err))
    WORST[entry, c.dtype] = max(WORST.get((entry, c.dtype), 0.0), ratio.max().item())
    bad = inside & ~(err <= bound)
    if bad.any():
        r, col = bad.nonzero()[0].tolist()
        raise AssertionError(f"{c.name}: {int(bad.sum())} elements outside the bound, first at (row {r}, column {col}): gate {g[r, col].item()}, got "
                             f"{got[r, col].item()}, want {want[r, col].item()}, |error| {err[r, col].item():.3e} > {bound[r, col].item():.3e}")
    pos, neg = g > G_TABLED, g < -G_TABLED
    lin = ref["lin"]
    lin_bound = lin.abs() * (u + (2.0 ** -24 if c.dtype == "bf16" else 0.0) + (1 + g.abs()) * torch.exp(-g.abs())) + floor
    bad = pos & ~((got - lin).abs() <= lin_bound)
    if bad.any():
        r, col = bad.nonzero()[0].tolist()
        raise AssertionError(f"{c.name}: gate {g[r, col].item()} at (row {r}, column {col}): got {got[r, col].item()}, one rounding of {lin[r, col].item()} expected")
    neg_bound = want.abs() * (1 + u + ref["const"] * g.abs() / G_TABLED) + floor
    bad = neg & ~(got.abs() <= neg_bound)
    if bad.any():
        r, col = bad.nonzero()[0].tolist()
        raise AssertionError(f"{c.name}: gate {g[r, col].item()} at (row {r}, column {col}): |{got[r, col].item()}| exceeds |reference| {want[r, col].abs().item()} + floor")


# (a pass stride short by one block is no mutation here: these kernels are not in place, a second visit stores the same value)
SWIGLU_MUTATIONS = ("gate_up_swapped", "du_halves_swapped", "dsilu_is_sigmoid", "dsilu_is_silu", "pad_column_written", "later_passes_skipped",
                    "last_partial_block_dropped", "slice_skipped", "slice_stride_2F", "ld_out_ignored", "lddu_is_ldu", "lddh_is_F")


def _silu_pair(g, mutation):
    s = 1.0 / (1.0 + torch.exp(-g))
    silu = g * s
    ds = s * (1.0 + g * (1.0 - s))
    if mutation == "dsilu_is_sigmoid":
        ds = s
    if mutation == "dsilu_is_silu":
        ds = silu
    return silu, ds


def emulate_swiglu(c: SwigluCase, win: dict, mutation: Optional[str] = None):
    """swiglu_fwd_kernel / swiglu_bwd_kernel (grid-stride passes over items of 4 columns) and swiglu_splitk_kernel (one item per thread)."""
    ob, ov = win["out"]
    O = ob.double()
    off, ldo = ov.storage_offset(), ov.stride(0)
    F, nq = c.F, c.F // 4
    q = _idx(4)[None, :]
    if c.kind == "splitk":
        P = win["part"][0].double()
        N2 = 2 * F
        slice_ = N2 if mutation == "slice_stride_2F" else c.rows * N2
        if mutation == "ld_out_ignored":
            ldo = F
        idx = _idx(c.rows * nq)
        m, col = idx // nq, ((idx % nq) * 4)[:, None] + q
        def sums(at):
            acc = torch.zeros(col.shape, dtype=torch.float64)
            for s in range(c.ks):
                if mutation == "slice_skipped" and s == 1:
                    continue
                acc = acc + _take(P, s * slice_ + (m * N2)[:, None] + at)
            return acc
        g, w = sums(col), sums(F + col)
        if mutation == "gate_up_swapped":
            g, w = w, g
        _put(O, off + (m * ldo)[:, None] + col, _round(_silu_pair(g, None)[0] * w, c.dtype))
        ob.copy_(O)
        return
    Uf = win["u"][0].double()
    ldu = win["u"][1].stride(0)
    if c.kind == "bwd":
        Df = win["dh"][0].double()
        lddh = F if mutation == "lddh_is_F" else win["dh"][1].stride(0)
        if mutation == "lddu_is_ldu":
            ldo = ldu
    for idx in _passes(c.items, mutation):
        r = idx // nq
        col = ((idx - r * nq) * 4)[:, None] + q
        g, b = _take(Uf, (r * ldu)[:, None] + col), _take(Uf, (r * ldu)[:, None] + F + col)
        if mutation == "gate_up_swapped":
            g, b = b, g
        silu, ds = _silu_pair(g, mutation)
        at = off + (r * ldo)[:, None] + col
        if c.kind == "fwd":
            _put(O, at, _round(silu * b, c.dtype))
            if mutation == "pad_column_written":
                _put(O, off + r * ldo + F, 0.0)
        else:
            d = _take(Df, (r * lddh)[:, None] + col)
            first, second = d * b * ds, d * silu
            if mutation == "du_halves_swapped":
                first, second = second, first
            _put(O, at, _round(first, c.dtype))
            _put(O, at + F, _round(second, c.dtype))
    ob.copy_(O)


ROPE_CASES = _build_rope_cases()
FINISH_CASES = _build_finish_cases()
SWIGLU_CASES = _build_swiglu_cases()
BY_NAME = {c.name: c for c in ROPE_CASES + FINISH_CASES + SWIGLU_CASES}
assert len(BY_NAME) == len(ROPE_CASES) + len(FINISH_CASES) + len(SWIGLU_CASES), "case names must be unique"
