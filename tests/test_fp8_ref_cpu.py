"""Host only: pins tests/_fp8_ref.py - the float64 reference the GPU probes of the row-wise e4m3 quantiser are held to
(tests/test_fp8_quantize_probe_gpu.py) - to torch's float8_e4m3fn, checks the facts its constructed rows rest on and the conditions on its
inputs, and shows on the CPU what the contract says of the kernels' arithmetic: the arithmetic before the scale floor (``mirror_parent``)
violates it on the rows below the floor, the arithmetic with the floor (``mirror``) satisfies it on every table, and each value-only mutant
of the GPU file's mutation table is flagged on the case that table names for it."""
import numpy as np
import pytest
import torch

import _fp8_ref as R

F32, BF16 = torch.float32, torch.bfloat16


def torch_encode(v32):
    """float32 values -> bytes by torch's cast (its NaN is 0x7F / 0xFF like the reference's)."""
    return torch.from_numpy(np.asarray(v32, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ------------------------------------------------------------------------------------------------------------------ the number format
def test_decode_is_torchs_for_every_non_nan_byte():
    b = np.array([v for v in range(256) if v & 0x7F != 0x7F], dtype=np.uint8)
    assert len(b) == 254
    want = torch.from_numpy(b).view(torch.float8_e4m3fn).double().numpy()
    got = R.e4m3_decode(b)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    assert np.isnan(R.e4m3_decode(np.array([0x7F, 0xFF]))).all()
    assert R.POS[-1] == 448.0 and R.POS[1] == 2.0 ** -9 and R.POS[8] == 2.0 ** -6 and (np.diff(R.POS) > 0).all()


def test_encode_is_torchs_cast_on_codes_midpoints_and_their_neighbours():
    codes = np.concatenate([R.POS, -R.POS])
    mids = np.concatenate([R.MID, -R.MID]).astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), np.concatenate([R.MID, -R.MID]))           # every midpoint is an fp32 value
    below, above = np.nextafter(mids, np.float32(0)), np.nextafter(mids, np.copysign(np.float32(np.inf), mids))
    edge = np.array([449.0, 463.9, 464.0, -449.0, -463.9, -464.0], dtype=np.float32)
    for v in (codes.astype(np.float32), mids, below, above, edge):
        assert np.array_equal(R.e4m3_encode(v.astype(np.float64)), torch_encode(v))
    assert np.array_equal(R.e4m3_encode(codes), np.concatenate([np.arange(0x7F), np.arange(0x7F) | 0x80]))   # encode(decode(b)) == b
    # 464 is the tie of 448 (even mantissa) and what would be 480: it rounds DOWN; anything above it rounds above 448, which is 0x7F
    over = float(np.nextafter(np.float32(464), np.float32(500)))
    assert R.e4m3_encode(np.array([449.0, 463.9, 464.0, -464.0, over, -over, 1e9, np.inf, -np.inf])).tolist() == [
        0x7E, 0x7E, 0x7E, 0xFE, 0x7F, 0xFF, 0x7F, 0x7F, 0xFF]
    assert torch_encode([over, -over, 1e9]).tolist() == [0x7F, 0xFF, 0x7F]
    # ties go to the even code, one fp32 ulp either side of a tie goes to that side's code
    lo, hi = np.arange(0x7E), np.arange(1, 0x7F)
    assert np.array_equal(R.e4m3_encode(R.MID), np.where(lo % 2 == 0, lo, hi))
    assert np.array_equal(R.e4m3_encode(below[:126].astype(np.float64)), lo) and np.array_equal(R.e4m3_encode(above[:126].astype(np.float64)), hi)


def test_encode_is_torchs_cast_on_random_values():
    g = torch.Generator().manual_seed(3)
    v = (torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-12, 9, (1 << 16,), generator=g).float())).numpy()
    assert np.array_equal(R.e4m3_encode(v.astype(np.float64)), torch_encode(v))


def test_spec_of_a_small_row():
    q, s = R.spec([[448.0, -224.0, 0.0, 1.0], [0.0, -0.0, 0.0, 0.0]])
    assert s.tolist() == [1.0, 1.0] and q.tolist() == [[0x7E, 0xF6, 0x00, 0x38], [0x00, 0x80, 0x00, 0x00]]


# ------------------------------------------------------------------------------------------ the facts the constructed rows rest on
def test_power_of_two_rows_have_exact_arithmetic():
    """amax = 448 * 2^k: fl32(amax * fl32(1/448)) is exactly 2^k for every k in [-126, 119] - so the reciprocal is 2^-k and x * 2^-k is
    exact for every x of the row (|x| <= amax: the product is at most 448 and no smaller than x's own precision allows)."""
    k = np.arange(-126, 120)
    amax = (np.float32(448.0) * np.exp2(k.astype(np.float64))).astype(np.float32)
    assert np.array_equal(amax.astype(np.float64), 448.0 * np.exp2(k.astype(np.float64))) and np.isfinite(amax).all()
    scale = amax * R.INV448_F32
    assert scale.dtype == np.float32 and np.array_equal(scale.astype(np.float64), np.exp2(k.astype(np.float64)))
    inv = np.float32(1.0) / scale
    assert np.array_equal(inv.astype(np.float64), np.exp2(-k.astype(np.float64)))
    for kk in R.TIE_EXPONENTS + (-126,):
        assert R.contract_scale(448.0 * 2.0 ** kk) == 2.0 ** kk
    assert R.contract_scale(0.0) == 1.0 and R.contract_scale(3 * R.FLOOR) == R.FLOOR and R.contract_scale(1e-36) == R.FLOOR
    assert R.contract_scale(float(np.nextafter(np.float32(R.UNFLOORED), np.float32(0)))) == R.FLOOR


def test_tie_tables_hold_what_they_say():
    f, b = R.tie_values(F32), R.tie_values(BF16)
    assert len(f) == 126 * 6 + 7 and len(b) == 126 * 2 + 7                     # bf16 holds every midpoint (5 significant bits)
    for t in (f, b):
        assert {2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6 - 2.0 ** -10, 448.0, -448.0} <= set(t)
        assert sum(1 for v in t if v == 0 and np.signbit(v)) == 1 and sum(1 for v in t if v == 0 and not np.signbit(v)) == 1
    for _, kernel, dtype, cols, *_ in R.VALUE_SHAPES:
        for k in R.TIE_EXPONENTS:
            x = R.f64(R.tie_row(k, dtype, cols))
            q, s = R.spec(x)
            assert s[0] == 2.0 ** k and np.array_equal(q, R.e4m3_encode(x * 2.0 ** -k))
        x = R.f64(R.first_unfloored_row(dtype, cols))
        assert np.abs(x).max() == R.UNFLOORED and ((x == 0) | (np.abs(x) >= R.FLOOR)).all()


# -------------------------------------------------------------------------------------------------- conditions on the chosen inputs
def all_finite_tables():
    """(name, kernel, x as float64, allow) for every finite-row input of the GPU probes."""
    for case in R.PATH_CASES:
        for rows in (1, 5):
            for turn in range(4):
                yield f"{case[0]}-{rows}-{turn}", case[1], R.f64(R.path_input(case, rows, turn)), True
    for name, kernel, dtype, cols, *_ in R.VALUE_SHAPES:
        for k in R.TIE_EXPONENTS:
            yield f"tie-{name}-{k}", kernel, R.f64(R.tie_row(k, dtype, cols)), False
        yield f"sweep-{name}", kernel, R.f64(R.sweep_rows(dtype, cols)), True
        yield f"tiny-{name}", kernel, R.f64(R.tiny_rows(dtype, cols)), False
        yield f"unfloored-{name}", kernel, R.f64(R.first_unfloored_row(dtype, cols)), False


def test_path_table_is_the_dispatch():
    for name, kernel, dtype, cols, ldx, cx, ld_out, co in R.PATH_CASES + R.VALUE_SHAPES:
        esz = 4 if dtype == F32 else 2
        assert cols % 4 == 0 and ldx % 4 == 0 and ld_out % 4 == 0 and cx + cols <= ldx and co + cols <= ld_out and (ldx > cols or ld_out > cols), name
        assert R.route(dtype, cols, ldx, ld_out, cx * esz, co) == kernel, name
        # every row of x starts at the alignment of the loads its kernel issues (16 bytes: float4 / bf16x8; 8: bf16x4); out likewise (8 / 4)
        load = 16 if dtype == F32 or kernel == "reg" else 8
        assert (cx * esz) % load == 0 and (ldx * esz) % load == 0 and co % (8 if kernel == "reg" else 4) == 0, name
    nv = lambda cols: (cols // 8 + 255) // 256
    assert sorted({1 if nv(c[3]) <= 1 else 2 if nv(c[3]) <= 2 else 4 if nv(c[3]) <= 4 else 8 for c in R.PATH_CASES if c[1] == "reg"}) == [1, 2, 4, 8]
    for _, kernel, _, cols, *_ in R.PATH_CASES:
        w = 4 if kernel == "generic" else 8
        first, last, wave3, second = R.places(cols, kernel)
        assert (first, last) == (0, cols - 1)
        if cols > 256 * w:
            assert wave3 // w >= 192 and wave3 < 256 * w and second >= 256 * w and (second // w) % 256 != 255
    assert any(c[3] % 8 == 0 and R.places(c[3], "reg")[1] % 8 == 7 for c in R.PATH_CASES if c[1] == "reg")


def test_inputs_meet_the_conditions_of_the_contract():
    """From the reference alone: at most 0.1 % of the elements of any case lie within the allowance window of a tie (so the allowance
    cannot carry a wrong kernel), no element of a row that is checked exactly or with the allowance is an fp32 subnormal, and the
    constructed rows need no allowance at all."""
    for name, _, x, allow in all_finite_tables():
        assert R.near_tie_share(x) <= R.MAX_TIE_SHARE or not allow, name
        assert ((x == 0) | (np.abs(x) >= R.FLOOR)).all(), name
        if not allow:                       # exact rows: scale a power of two (or floored), quotients exact
            for r in x:
                assert np.log2(R.contract_scale(np.abs(r).max())) % 1 == 0, name
    g = R.f64(R.gauss(64, 4096, 1, F32))
    assert R.near_tie_share(g) <= 1e-4      # what a Gaussian matrix gives: a few elements in a million


# ------------------------------------------------------------------- the kernels' arithmetic against the contract, without a GPU
def test_the_arithmetic_before_the_floor_breaks_the_contract_on_tiny_rows():
    q, s = R.mirror_parent(np.array([[1e-36, -5e-37, 3.3e-37, 0.0]]))
    assert q.tolist() == [[0x7F, 0xFF, 0x7F, 0x7F]] or q.tolist() == [[0x7F, 0xFF, 0x7F, 0xFF]]      # every element NaN, the exact zero too
    for name, kernel, dtype, cols, *_ in R.VALUE_SHAPES:
        x = R.f64(R.tiny_rows(dtype, cols))
        q, s = R.mirror_parent(x, kernel)
        bad = R.check_rows(x, q, s, allow=False)
        assert any("row 0" in m and "NaN byte" in m for m in bad) and any("row 1" in m and "NaN byte" in m for m in bad), (name, bad)
        assert any("scale" in m for m in bad)
        # ... and on nothing else: the floor changes no row from 448 * 2^-126 up
        for other, allow in ((R.first_unfloored_row(dtype, cols), False), (R.sweep_rows(dtype, cols), True), (R.tie_row(-20, dtype, cols), False)):
            x = R.f64(other)
            assert R.check_rows(x, *R.mirror_parent(x, kernel), allow=allow) == []
            assert all(np.array_equal(a, b) for a, b in zip(R.mirror_parent(x, kernel), R.mirror(x, kernel)))


def test_the_arithmetic_with_the_floor_meets_the_contract_on_every_table():
    stats = {}
    for name, kernel, x, allow in all_finite_tables():
        q, s = R.mirror(x, kernel)
        assert R.check_rows(x, q, s, allow=allow, stats=stats) == [], name
    assert stats["allowed"] <= R.MAX_TIE_SHARE * stats["elements"]
    for name, kernel, dtype, cols, *_ in R.VALUE_SHAPES:
        x = R.f64(R.tiny_rows(dtype, cols))
        q, s = R.mirror(x, kernel)
        assert s.tolist() == [R.FLOOR, R.FLOOR] and np.array_equal(q[0], R.e4m3_encode(np.arange(cols) % 7 - 3.0))
        for last in (False, True):
            x, clean = (R.f64(t) for t in R.poisoned_rows(dtype, cols, last))
            q, s = R.mirror(x, kernel)
            qc, sc = R.mirror(clean, kernel)
            assert R.check_rows(x, q, s) == []
            for r in range(5):
                if r not in R.POISONED:
                    assert np.array_equal(q[r], qc[r]) and s[r] == sc[r]
        x = R.f64(R.subnormal_row(dtype, cols))
        q, s = R.mirror(x, kernel)
        assert s[0] == R.FLOOR and not ((q & 0x7F) == 0x7F).any() and (np.abs(R.e4m3_decode(q) * R.FLOOR - x) <= R.FLOOR).all()


def test_check_row_names_what_is_wrong():
    x = np.array([448.0, -224.0, 0.0, -0.0, 1.0, 17.0, 3.0, 100.0])
    q, s = R.spec(x)
    assert R.check_row(x, q[0], 1.0) == []
    assert any("scale" in m for m in R.check_row(x, q[0], float(np.nextafter(np.float32(1), np.float32(2)))))
    for i, byte, word in ((2, 0x80, "zero"), (3, 0x00, "zero"), (0, 0x7D, "amax"), (4, 0x39, "ideal"), (5, 0x7F, "NaN byte")):
        got = q[0].copy()
        got[i] = byte
        assert any(word in m for m in R.check_row(x, got, 1.0)), (i, word)
    # the neighbour is accepted only inside the window: 17 is a tie of 16 and 18 (codes 0x58, 0x59)
    x = np.array([448.0, 17.0, 17.0 * (1 + 2.0 ** -20), 17.0 * (1 + 2.0 ** -22), 0.0, 0.0, 0.0, 0.0])
    q = R.spec(x)[0][0]
    assert q[1:4].tolist() == [0x58, 0x59, 0x59]
    lower = q.copy(); lower[2] = 0x58
    assert R.check_row(x, lower, 1.0) != []
    lower = q.copy(); lower[3] = 0x58
    st = {}
    assert R.check_row(x, lower, 1.0, stats=st) == [] and st == {"elements": 8, "allowed": 1, "exact_ties": 0}
    assert R.check_row(x, lower, 1.0, allow=False) != []
    upper = q.copy(); upper[1] = 0x59
    assert R.check_row(x, upper, 1.0, stats=st) == [] and st["exact_ties"] == 1 and R.check_row(x, upper, 1.0, allow=False) != []
    # a non-finite input must not come back finite
    x = np.array([np.nan, 1.0, np.inf, 2.0])
    assert R.check_row(x, np.array([0x7F, 0x10, 0xFF, 0x20]), 1.0) == []
    assert R.check_row(x, np.array([0x00, 0x00, 0x00, 0x00]), np.inf) == []
    assert R.check_row(x, np.array([0x7F, 0x10, 0x7E, 0x20]), 1.0) != []


# (mutant, the probe that catches it: table, shape, what of that table) - the header of tests/test_fp8_quantize_probe_gpu.py
MUTANT_CASES = [
    ("first_pass_only", "generic-f32-1028", 1, 3),        # the maximum in the second pass (rows = 1, turn 3: place 3)
    ("first_pass_only", "generic-bf16-2052", 5, 0),
    ("no_red3", "generic-f32-1020", 1, 2),                # the maximum in the last wave's share
    ("no_red3", "reg-bf16-2048", 1, 2),
    ("skip_elem7", "reg-bf16-2048", 1, 1),                # the maximum in the last column, element 7 of its vector
    ("skip_elem7", "reg-bf16-8", 1, 1),
    ("swap_words", "generic-f32-4", 1, 0),
    ("swap_words", "reg-bf16-8", 5, 0),
    ("scale_thread0", "generic-f32-1024", 1, 1),
    ("scale_thread0", "reg-bf16-16384", 5, 0),
]


@pytest.mark.parametrize("mutant,case_id,rows,turn", MUTANT_CASES)
def test_each_value_mutant_is_flagged_on_its_case(mutant, case_id, rows, turn):
    case = next(c for c in R.PATH_CASES if c[0] == case_id)
    x = R.f64(R.path_input(case, rows, turn))
    assert R.check_rows(x, *R.mirror(x, case[1])) == []
    assert R.check_rows(x, *R.mirror(x, case[1], mutant)) != []


def test_the_removed_floor_is_flagged_on_the_tiny_rows_only():
    for name, kernel, x, allow in all_finite_tables():
        bad = R.check_rows(x, *R.mirror(x, kernel, "no_floor"), allow=allow)
        assert (bad != []) == name.startswith("tiny-"), (name, bad[:2])
