"""An independent reference of the row-wise e4m3 quantiser (eavqa_quantize_rows_fp8 and its fused twins eavqa_layernorm_fwd_fp8 / _bwd_fp8 /
_splitk_fp8): plain float64 and integers.  Nothing here calls torch.float8_e4m3fn (tests/test_fp8_ref_cpu.py pins the encoder and the
decoder to it) and nothing restates the kernels' reciprocal: the expected code of an element is encode(x / (amax / 448)) in float64
(``quotient``: x * 448 / amax, one rounding).

The contract (``check_row``; the header of csrc/gemm_fp8.hip states the same):

  a row whose elements are all finite
    * scale is a finite, positive, normal fp32: 1.0 exactly for an all-zero row, else max(fl32(amax * fl32(1/448)), 2^-126) - so
      |scale - amax / 448| <= 2^-23 scale whenever amax >= 448 * 2^-126 (two roundings of half an ulp each);
    * no byte is 0x7F / 0xFF; a zero element gives 0x00 / 0x80 with its sign; when amax >= 448 * 2^-126 an element of magnitude amax gives
      0x7E / 0xFE;
    * every byte is the float64 ideal code.  The code NEXT to it is accepted only where the float64 quotient lies within a relative 2^-21
      of the midpoint between the two (scale, reciprocal and product round half an fp32 ulp each: under 2^-22, doubled).  How many elements
      of a case may sit that close to a midpoint is a condition on the case, not a measurement: at most 0.1 % (``near_tie_share``, asserted
      for every input below by tests/test_fp8_ref_cpu.py);
    * a row below the floor (0 < amax < 448 * 2^-126) has scale 2^-126 and the bytes encode(x * 2^126): that product is exact, so such a
      row - like the tie rows, whose scale is a power of two - gets no allowance (``allow=False``).
  a row that holds a NaN or an infinity
    * the dequantised element at every non-finite position is non-finite (the other clause - the other rows of the call do not change -
      takes two calls and lives in the GPU test).

``mirror`` is the kernels' fp32 arithmetic on the CPU, with the value-only mutations of tests/test_fp8_quantize_probe_gpu.py's header;
``mirror_parent`` is that arithmetic before the scale floor existed.  The case tables at the end are shared by the CPU and the GPU test."""
import numpy as np
import torch

E4M3_MAX = 448.0
FLOOR = 2.0 ** -126                       # the smallest normal fp32: the floor of a row scale
UNFLOORED = E4M3_MAX * FLOOR              # rows with amax >= this are not touched by the floor
INV448_F32 = np.float32(1.0) / np.float32(448.0)
TIE_WINDOW = 2.0 ** -21
MAX_TIE_SHARE = 1e-3


# ------------------------------------------------------------------------------------------------------------------ the number format
def e4m3_decode(b):
    """OCP e4m3fn byte(s) -> float64 (0x7F / 0xFF: NaN)."""
    b = np.asarray(b).astype(np.int64)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * np.exp2((e - 7).astype(np.float64)))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return np.where(b >> 7 == 1, -mag, mag)


def e4m3_encode(v):
    """float64 -> OCP e4m3fn byte(s), round to nearest even: spacing 2^(e-3) in the binade of 2^e, 2^-9 below 2^-6; a rounded magnitude
    above 448 (and a NaN) is 0x7F with the sign bit."""
    a = np.asarray(v, dtype=np.float64)
    sign = np.signbit(a).astype(np.int64) << 7
    mag = np.abs(a)
    fin = np.isfinite(mag)
    m = np.where(fin, mag, 0.0)
    e = np.maximum(np.frexp(m)[1].astype(np.int64) - 1, -6)          # m = f 2^(e+1), f in [0.5, 1); subnormals share the spacing of 2^-6
    n = np.rint(np.ldexp(m, (3 - e).astype(np.int32))).astype(np.int64)   # units of 2^(e-3): exact scaling, then RNE (np.rint)
    carry = n == 16
    e, n = np.where(carry, e + 1, e), np.where(carry, 8, n)
    byte = np.where(n < 8, n, ((e + 7) << 3) + (n - 8))               # n < 8: subnormal codes (e = -6) and zero
    over = ~fin | (e > 8) | ((e == 8) & (n > 14))
    return (np.where(over, 0x7F, byte) | sign).astype(np.uint8)


POS = e4m3_decode(np.arange(0x7F))        # the 127 non-negative codes, ascending with the byte
MID = (POS[:-1] + POS[1:]) / 2            # the 126 midpoints between adjacent codes


def spec(x):
    """Per row of ``x`` (float64 [rows, cols], finite): (ideal codes, ideal scale) with amax = max|x|, scale = amax / 448 (1 for a zero row)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    amax = np.abs(x).max(axis=1)
    scale = np.where(amax > 0, amax / E4M3_MAX, 1.0)
    return e4m3_encode(quotient(x, amax[:, None])), scale


def quotient(x, amax):
    """x / (amax / 448) as ONE float64 rounding: x * 448 is exact (27 bits at most for an fp32 x), so the division returns the correctly
    rounded quotient - and a quotient that IS a midpoint of two codes (bf16 rows have many) comes out as that midpoint exactly."""
    with np.errstate(all="ignore"):
        return np.where(amax > 0, x * E4M3_MAX / np.where(amax > 0, amax, 1.0), x)


def contract_scale(amax):
    """max(fl32(amax * fl32(1/448)), 2^-126), 1 for amax == 0 (amax: an fp32 value held in float64)."""
    if amax == 0:
        return 1.0
    with np.errstate(all="ignore"):
        return max(float(np.float32(amax) * INV448_F32), FLOOR)


def tie_distance(quo):
    """Relative distance of |quo| (float64 quotients x / (amax / 448)) to the nearest midpoint between two adjacent codes."""
    q = np.abs(np.asarray(quo, dtype=np.float64))
    j = np.clip(np.searchsorted(MID, q), 1, len(MID) - 1)
    lo, hi = MID[j - 1], MID[j]
    return np.minimum(np.abs(q - lo) / lo, np.abs(q - hi) / hi)


def near_tie_share(x):
    """Share of the elements of ``x`` (finite rows at or above the floor) whose ideal quotient lies inside the allowance window."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    amax = np.abs(x).max(axis=1)
    rows = amax >= UNFLOORED
    quo = quotient(x[rows], amax[rows][:, None])
    return float((tie_distance(quo) <= TIE_WINDOW).sum()) / max(1, x.size)


def _some(idx, limit=4):
    idx = np.flatnonzero(idx)
    return f"{len(idx)} element(s), first at {idx[:limit].tolist()}"


def check_row(x_row, q_row, scale, allow=True, stats=None):
    """The contract above for one row: the violations, as a list of strings (empty: the row conforms).  ``stats`` (a dict) counts the
    elements seen, those that needed the neighbour allowance and, of these, the ones whose float64 quotient IS the midpoint."""
    x = np.asarray(x_row, dtype=np.float64).ravel()
    q = np.asarray(q_row).astype(np.uint8).ravel()
    s = float(scale)
    assert x.shape == q.shape
    bad = []
    if not np.isfinite(x).all():
        with np.errstate(all="ignore"):
            back = e4m3_decode(q) * s
        leak = ~np.isfinite(x) & np.isfinite(back)
        if leak.any():
            bad.append(f"a non-finite input became a finite number: {_some(leak)}")
        return bad
    amax = float(np.abs(x).max())
    if not (np.isfinite(s) and s >= FLOOR):
        bad.append(f"scale {s!r} is not a finite positive normal fp32")
    want = contract_scale(amax)
    if s != want:
        bad.append(f"scale {s!r}, the rule gives {want!r} (amax {amax!r})")
    if amax >= UNFLOORED and not abs(s - amax / E4M3_MAX) <= 2.0 ** -23 * s:
        bad.append(f"scale {s!r} is further than 2^-23 from amax / 448 = {amax / E4M3_MAX!r}")
    nan = (q & 0x7F) == 0x7F
    if nan.any():
        bad.append(f"NaN byte in a finite row: {_some(nan)}")
    zero = (x == 0) & (q != np.where(np.signbit(x), 0x80, 0x00))
    if zero.any():
        bad.append(f"a zero did not stay a zero of its sign: {_some(zero)}")
    used = exact = 0
    if amax > 0 and amax < UNFLOORED:
        wrong = q != e4m3_encode(np.ldexp(x, 126))                    # below the floor: x * 2^126, exact
        if wrong.any():
            bad.append(f"bytes of a floored row differ from encode(x * 2^126): {_some(wrong)}")
    elif amax > 0:
        top = (np.abs(x) == amax) & (q != np.where(np.signbit(x), 0xFE, 0x7E))
        if top.any():
            bad.append(f"an element of magnitude amax is not 0x7E / 0xFE: {_some(top)}")
        quo = quotient(x, amax)
        ideal = e4m3_encode(quo)
        off = np.flatnonzero(q != ideal)
        wrong = np.zeros(x.shape, dtype=bool)
        for i in off:
            a, b = int(ideal[i]), int(q[i])
            neighbour = (a ^ b) < 0x80 and abs((a & 0x7F) - (b & 0x7F)) == 1 and (b & 0x7F) != 0x7F
            mid = (POS[a & 0x7F] + POS[b & 0x7F]) / 2 if neighbour else np.inf
            if allow and neighbour and abs(abs(quo[i]) - mid) <= TIE_WINDOW * mid:
                used += 1
                exact += abs(quo[i]) == mid
            else:
                wrong[i] = True
        if wrong.any():
            i = int(np.flatnonzero(wrong)[0])
            bad.append(f"bytes differ from the ideal code: {_some(wrong)} (x {x[i]!r}, quotient {quo[i]!r}, got 0x{q[i]:02X}, ideal 0x{ideal[i]:02X})")
    if stats is not None:
        stats["elements"] = stats.get("elements", 0) + x.size
        stats["allowed"] = stats.get("allowed", 0) + used
        stats["exact_ties"] = stats.get("exact_ties", 0) + int(exact)
    return bad


def check_rows(x, q, scale, allow=True, stats=None):
    """``check_row`` on every row of a matrix; each violation carries its row."""
    x, q, scale = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.atleast_2d(np.asarray(q)), np.asarray(scale, dtype=np.float64).ravel()
    assert x.shape == q.shape and scale.shape == (x.shape[0],)
    return [f"row {r}: {m}" for r in range(x.shape[0]) for m in check_row(x[r], q[r], scale[r], allow, stats)]


# -------------------------------------------------------------------------------------------- the kernels' arithmetic on the CPU, mutants
MUTANTS = ("first_pass_only", "no_red3", "skip_elem7", "swap_words", "no_floor", "scale_thread0")


def route(dtype, cols, ldx, ld_out, x_off_bytes=0, out_off_bytes=0):
    """The dispatch of eavqa_quantize_rows_fp8 (csrc/gemm.hip), restated: which kernel a call reaches."""
    reg = (dtype == torch.bfloat16 and cols % 8 == 0 and cols <= 16384 and ldx % 8 == 0 and ld_out % 8 == 0
           and x_off_bytes % 16 == 0 and out_off_bytes % 8 == 0)
    return "reg" if reg else "generic"


def _rule(amax, floor=True):
    with np.errstate(all="ignore"):
        if not amax > 0:
            return np.float32(1.0)
        s = np.float32(amax) * INV448_F32
        return max(s, np.float32(FLOOR)) if floor else s


def mirror(x, kernel="generic", mutant=None):
    """(bytes, scales) as the kernels compute them in fp32 (``kernel``: which thread owns which column - 4 per thread and 1024 per pass in the
    generic kernel, 8 and 2048 in the register kernel).  ``mutant``: one of MUTANTS, the value-only mutations of the GPU probes' header."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    rows, cols = x.shape
    w = 4 if kernel == "generic" else 8
    c = np.arange(cols)
    thread, pas = (c // w) % 256, c // (256 * w)
    keep = {"first_pass_only": pas == 0, "no_red3": thread < 192, "skip_elem7": c % 8 != 7}.get(mutant, np.ones(cols, dtype=bool))
    q, sc = np.zeros((rows, cols), dtype=np.uint8), np.zeros(rows, dtype=np.float32)
    with np.errstate(all="ignore"):
        for r in range(rows):
            a = np.abs(x[r])
            scale = _rule(np.fmax.reduce(a[keep], initial=np.float32(0)), floor=mutant != "no_floor")      # fmaxf drops a NaN
            inv = np.float32(1.0) / scale
            b = e4m3_encode((x[r] * inv).astype(np.float64))
            if mutant == "swap_words":
                b = b.reshape(-1, 4)[:, [2, 3, 0, 1]].ravel()
            q[r] = b
            sc[r] = _rule(np.fmax.reduce(a[thread == 0], initial=np.float32(0))) if mutant == "scale_thread0" else scale
    return q, sc


def mirror_parent(x, kernel="generic"):
    """The arithmetic before the floor: scale = amax * (1/448) however small, inv = 1 / scale."""
    return mirror(x, kernel, "no_floor")


# ------------------------------------------------------------------------------------------------------------------------- case tables
F32, BF16 = torch.float32, torch.bfloat16


def f64(t):
    return t.double().numpy()


def gauss(rows, cols, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g).to(dtype)


# (id, kernel, dtype, cols, ldx, first column of x in its wider matrix, ld_out, first column of out): x starts 16 bytes aligned for f32 and
# for the register kernel, 8 bytes for the generic kernel's bf16 rows; out 8 / 4 bytes.  Every case runs with 1 and with 5 rows.
def _path_cases():
    cases = []
    for cols in (4, 1020, 1024, 1028, 2052):
        cases.append((f"generic-f32-{cols}", "generic", F32, cols, cols + 4, 4, cols + 8, 4))
    for cols in (4, 12, 1020, 1028, 2052):                                        # bf16 rows whose length is no multiple of 8
        cases.append((f"generic-bf16-{cols}", "generic", BF16, cols, cols + 4, 4, cols + 8, 4))
    cases.append(("generic-bf16-16392", "generic", BF16, 16392, 16400, 8, 16408, 8))            # by the row length alone
    cases.append(("generic-bf16-1024-ldx", "generic", BF16, 1024, 1028, 0, 1040, 8))             # by the input stride alone
    cases.append(("generic-bf16-1024-ldout", "generic", BF16, 1024, 1032, 8, 1028, 0))           # by the output stride alone
    for cols in (8, 2048, 2056, 4096, 4104, 8192, 8200, 16384):                   # NV = 1, 1, 2, 2, 4, 4, 8, 8
        cases.append((f"reg-bf16-{cols}", "reg", BF16, cols, cols + 8, 8, cols + 16, 8))
    return cases


PATH_CASES = _path_cases()
# The planted maximum: above every |Gaussian| drawn here and a bf16 value, 251 / 32 with 251 prime - a quotient x * 448 / PLANT of a bf16 x
# (8 significant bits) is then never a midpoint of two codes.  With a rounder maximum it often is (amax 7.5: x = 2.8125 gives 168 exactly,
# the tie of 160 and 176), and a case of a few elements would spend its whole allowance on ties that fp32 may break either way.
PLANT = 7.84375


def places(cols, kernel):
    """The four columns the row maximum is planted at: the first, the last, one that the LAST wave of the block owns in the first pass, one
    in the second pass (the middle column where the row is too short to have such a column)."""
    wave3, second = (900, 1026) if kernel == "generic" else (1807, 2053)
    return [0, cols - 1, wave3 if cols > wave3 else cols // 2, second if cols > second else cols // 2]


def path_input(case, rows, turn):
    """Gaussian rows with the maximum planted: row r of turn ``turn`` (0 .. 3) at place (r + turn) % 4, negative in every third one."""
    _, kernel, dtype, cols = case[:4]
    x = gauss(rows, cols, 100 + cols, dtype).clone()
    assert x.abs().max().item() < PLANT
    where = places(cols, kernel)
    for r in range(rows):
        x[r, where[(r + turn) % 4]] = -PLANT if (r + 2 * turn) % 3 == 0 else PLANT
    return x


# one shape per kernel for the value tables: (id, kernel, dtype, cols, ldx, x column, ld_out, out column)
VALUE_SHAPES = [("generic-f32", "generic", F32, 1028, 1032, 4, 1036, 4),
                ("generic-bf16", "generic", BF16, 1028, 1032, 4, 1036, 4),
                ("reg-bf16", "reg", BF16, 2056, 2064, 8, 2072, 8)]
TIE_EXPONENTS = (0, -20, 100)


def tie_values(dtype, least=0.0):
    """Every midpoint between adjacent codes in both signs (those the type represents), for fp32 also one ulp either side of each; +0, -0,
    the subnormal ties 2^-10 and 3 * 2^-10, 2^-6 - 2^-10, and +-448 (the row's amax).  ``least``: drop magnitudes below it."""
    t = []
    for m in MID:
        if float(torch.tensor(m, dtype=torch.float64).to(dtype).double()) != m:
            continue                                                              # (no e4m3 midpoint needs more than 5 bits: none is dropped)
        near = [m]
        if dtype == F32:
            near += [float(np.nextafter(np.float32(m), np.float32(0))), float(np.nextafter(np.float32(m), np.float32(np.inf)))]
        t += [s * v for v in near for s in (1.0, -1.0)]
    t += [0.0, -0.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6 - 2.0 ** -10, 448.0, -448.0]
    return [v for v in t if abs(v) >= least]


def tie_row(k, dtype, cols, least=0.0):
    """[1, cols]: 2^k * tie_values, then zeros.  amax = 448 * 2^k, so the scale is 2^k and every quotient is exact."""
    t = torch.tensor(tie_values(dtype, least), dtype=torch.float64) * 2.0 ** k
    assert len(t) <= cols
    row = torch.zeros(1, cols, dtype=torch.float64)
    row[0, :len(t)] = t
    assert torch.equal(row.to(dtype).double(), row)                                # every value is one the type holds
    return row.to(dtype)


SWEEP_EXPONENTS = tuple(range(-110, 111, 10))


def sweep_rows(dtype, cols):
    """Gaussian rows (their maximum PLANT, for the reason given there) times 2^k, k = -110 .. 110 in steps of 10, and a row whose amax is
    the largest finite value of the type."""
    g = gauss(len(SWEEP_EXPONENTS) + 1, cols, 7, dtype).double()
    g[:, 3] = PLANT * (1 - 2 * (torch.arange(g.shape[0]) % 2)).double()
    scale = torch.tensor([2.0 ** k for k in SWEEP_EXPONENTS] + [2.0 ** 120], dtype=torch.float64)
    x = g * scale[:, None]
    x[-1, 5] = -torch.finfo(dtype).max
    assert torch.equal(x.to(dtype).double(), x)
    return x.to(dtype)


def tiny_rows(dtype, cols):
    """Rows below the floor.  Row 0: 2^-126 * n, n = -3 .. 3 (scale 2^-126, bytes encode(n)); row 1: amax = 1e-36."""
    n = torch.arange(cols) % 7 - 3
    u = torch.tensor([1.0, -0.5, 0.33, 0.0, 0.75, -0.9, 0.02, 0.6], dtype=torch.float32)[torch.arange(cols) % 8]
    x = torch.stack([n.double() * FLOOR, (u * torch.tensor(1e-36, dtype=torch.float32)).to(dtype).double()])
    assert torch.equal(x.to(dtype).double(), x) and bool(((x == 0) | (x.abs() >= FLOOR)).all())
    return x.to(dtype)


def first_unfloored_row(dtype, cols):
    """amax = 448 * 2^-126 exactly: the first row the floor does not touch (the ties of magnitude >= 1, so that no element is subnormal)."""
    return tie_row(-126, dtype, cols, least=1.0)


def subnormal_row(dtype, cols):
    """fp32-subnormal elements under a normal maximum 2 * 2^-126.  A device may read them as zeros: only no NaN, scale 2^-126 and
    |dequantised - x| <= 2^-126 are asserted of this row."""
    v = torch.tensor([2.0, 0.5, -0.5, 0.25, 0.75, 2.0 ** -7, -2.0 ** -4, 0.0], dtype=torch.float64) * FLOOR
    x = v[torch.arange(cols) % 8][None]
    assert torch.equal(x.to(dtype).double(), x)
    return x.to(dtype)


def poisoned_rows(dtype, cols, last):
    """5 Gaussian rows; rows 0, 2, 4 hold a NaN, a +inf, a -inf (in the first column, or the last).  Returns (x, x with those rows zeroed)."""
    x = gauss(5, cols, 11, dtype).clone()
    clean = x.clone()
    for r, v in ((0, float("nan")), (2, float("inf")), (4, float("-inf"))):
        x[r, cols - 1 if last else 0] = v
        clean[r] = 0
    return x, clean


POISONED = (0, 2, 4)
