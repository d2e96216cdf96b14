"""GPU: the exact per-key probes of tests/_attention_probe.py through the attention code that generation and scoring stand on -
``eavqa_attention_decode_shared`` (every template form, strided q | k_new | v_new, garbage in every spare row and slot),
``eavqa_attention_merge`` alone (bit for bit) and behind its two ``attention_fwd`` segments, and the two decode entry points that take
their query from split-K partial sums (plain with a bias, cross-attention with and without a bias table).

The acceptance check is the one of test_attention_probe_gpu.py: |got - want| <= 2^-8 (abs_companion + |want|) + 1e-6 (1e-5 in fp32)
against a float64 reference, invisible keys read exactly zero.  tests/test_attention_probe_cpu.py shows that a kernel wrong in one
index (a neighbour's tail, slot t + 1, the mask stride, lse1 in lse2's layout, ...) would not pass."""
import pytest
import torch

import _attention_probe as ap
from test_attention_probe_gpu import BF16, DEV, F32, GARBAGE, WORST, _cache, _padded_mask, back, probes_and_refs, rows, setup

pytestmark = pytest.mark.gpu

SENTINEL = -7.0                                 # what the guard columns and the guard row around an output hold
FAMILIES = ("shared", "merge", "score flow", "decode from partial sums, plain", "decode from partial sums, cross")


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    yield _ops
    print("\nworst error / bound per kernel family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items()) if k.startswith(FAMILIES)))


def note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), worst)


def guarded(n_rows, width, dtype):
    """(the sentinel-filled buffer [n_rows + 1, width + 16], its window [n_rows, width] 8 columns in)."""
    wide = torch.full((n_rows + 1, width + 16), SENTINEL, dtype=dtype, device=DEV)
    return wide, wide[:n_rows, 8:8 + width]


def guards_intact(wide, n_rows, width):
    return bool((wide[n_rows] == SENTINEL).all() and (wide[:, :8] == SENTINEL).all() and (wide[:, 8 + width:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------- shared prompt
_SHARED = {}


def shared_probes_and_refs(sc):
    """[(probe, float64 reference, the call's buffers)] of a case, built once and never written to."""
    if sc not in _SHARED:
        keep = ap.shared_keep(sc)
        _SHARED[sc] = [(pr, ap.reference(pr.q, pr.k, pr.v, None, keep, None, pr.scale), ap.shared_buffers(sc, pr)) for pr in ap.shared_probes(sc)]
    return _SHARED[sc]


@pytest.mark.parametrize("sc", ap.SHARED_CASES, ids=[c.id for c in ap.SHARED_CASES])
def test_shared_prompt_decode_step(ops, sc):
    """attention_decode_shared: Probe A reads every (row, key) weight out with the factor of its head and, in the tail, of its row;
    Probe B selects the keys at the prompt batch edges and at both ends of the tail.  Spare prompt rows, spare tail slots and the
    stale slot t hold garbage; afterwards slot t holds the new row bit for bit and nothing else has moved."""
    B, G, H, S0, hd, t, dtype = sc.B, sc.G, sc.H, sc.S0, sc.hd, sc.n - 1, sc.torch_dtype
    R, E, pbr = B * G, H * hd, S0 + 3
    ok = torch.ones(R, 1, dtype=torch.bool)
    worst = 0.0
    for pr, ref, buf in shared_probes_and_refs(sc):
        what = f"{sc.id} {pr.name}"
        if pr.name.startswith("B"):
            assert bool(((ref.p == 1.0) | (ref.p < 1e-27)).all()), what                         # one-hot
        dev = {n: x.to(dtype).to(DEV) for n, x in buf.items() if n != "mask" and x is not None}
        mask = buf["mask"].to(DEV) if buf["mask"] is not None else None
        before = {n: dev[n].clone() for n in ("kp", "vp", "kt", "vt")}
        qkv = dev["qkv"]
        wide, out = guarded(R, E, dtype)
        got = ops.attention_decode_shared(qkv[:, :E], dev["kp"].view(B * pbr, E), dev["vp"].view(B * pbr, E), dev["kt"], dev["vt"], qkv[:, E:2 * E],
                                          qkv[:, 2 * E:], B, G, H, S0, t, hd, prompt_batch_rows=pbr, key_mask=mask,
                                          ld_mask=mask.stride(0) if mask is not None else 0, scale=pr.scale, out=out)
        assert got.data_ptr() == out.data_ptr() and qkv.stride(0) == 3 * E and out.stride(0) == E + 16
        worst = max(worst, ap.check({"o": back(out, R, 1, H, hd)}, ref, dtype, ok, pr.exact_zero, what=what))
        assert guards_intact(wide, R, E), what
        assert torch.equal(dev["kt"][:, t], qkv[:, E:2 * E]) and torch.equal(dev["vt"][:, t], qkv[:, 2 * E:]), what
        others = torch.arange(sc.t_max, device=DEV) != t
        assert torch.equal(dev["kt"][:, others], before["kt"][:, others]) and torch.equal(dev["vt"][:, others], before["vt"][:, others]), what
        assert torch.equal(dev["kp"], before["kp"]) and torch.equal(dev["vp"], before["vp"]), what
    family = f"shared {sc.dtype} {'hd > 64' if hd > 64 else 'hd <= 64'}"
    print(f"{family} {sc.id}: worst error / bound {worst:.3f}")
    note(family, worst)


# ------------------------------------------------------------------------------------------------------------------- merge alone
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", ap.MERGE_CASES, ids=["x".join(map(str, s)) for s in ap.MERGE_CASES])
def test_merge_picks_the_stated_segment_bit_for_bit(ops, shape, dtype):
    """attention_merge with weights that are exactly 0, 0.5 or 1 (and the four empty-segment kinds in one call): torch.equal against
    the construction, with three different row strides, guards around the output, and once more in place (out = o2)."""
    B, C, T, H, hd = shape
    N, E = B * C * T, H * hd
    for pattern in ap.MERGE_PATTERNS:
        o1, o2, l1, l2 = ap.merge_inputs(shape, pattern)
        want = ap.merge_expected(shape, o1, o2, l1, l2).to(dtype).to(DEV)
        w1, a = guarded(N, E + 8, dtype)                                                        # ld1 = E + 24, ld2 = E + 32, ldo = E + 16
        w2, b = guarded(N, E + 16, dtype)
        a, b = a[:, :E], b[:, :E]
        a.copy_(o1.to(dtype))
        b.copy_(o2.to(dtype))
        wide, out = guarded(N, E, dtype)
        assert len({a.stride(0), b.stride(0), out.stride(0)}) == 3 and min(a.stride(0), b.stride(0), out.stride(0)) > E
        keep_a, keep_b = a.clone(), b.clone()
        got = ops.attention_merge(a, l1.to(DEV), b, l2.to(DEV), B, C, T, H, hd, out=out)
        assert torch.equal(got, want), f"{shape} {pattern}: {int((got != want).sum())} elements differ"
        assert guards_intact(wide, N, E) and torch.equal(a, keep_a) and torch.equal(b, keep_b)
        inplace = ops.attention_merge(a, l1.to(DEV), b, l2.to(DEV), B, C, T, H, hd)
        assert inplace.data_ptr() == b.data_ptr() and torch.equal(b, want) and torch.equal(a, keep_a), f"{shape} {pattern} in place"
        assert guards_intact(w2, N, E) and guards_intact(w1, N, E)
    note("merge alone (exact)", 0.0)


# ------------------------------------------------------------------------------------------------------------------- score flow
_FLOW = {}


def flow_probes_and_refs(fc):
    if fc not in _FLOW:
        keep = ap.flow_keep(fc)
        _FLOW[fc] = [(pr, ap.reference(pr.q, pr.k, pr.v, None, keep, None, pr.scale)) for pr in ap.flow_probes(fc)]
    return _FLOW[fc]


@pytest.mark.parametrize("fc", ap.SCORE_FLOW_CASES, ids=[c.id for c in ap.SCORE_FLOW_CASES])
def test_score_flow_per_key(ops, fc):
    """attention_fwd over the shared, masked prompt + attention_fwd over each candidate's causal prefix + attention_merge, against one
    float64 attention over [masked prompt | causal prefix].  The bound is ap.check's as it stands: three roundings to the storage type
    stay inside it (test_score_flow_probes_and_the_three_roundings_stay_within_the_bound measured 0.807 at most for the emulation)."""
    B, C, T, S0, H, hd, dtype = fc.B, fc.C, fc.T, fc.S0, fc.H, fc.hd, fc.torch_dtype
    N, E = B * C, H * hd
    mask = ap.flow_mask(fc).to(DEV)
    ok = torch.ones(N, T, dtype=torch.bool)
    worst = 0.0
    for pr, ref in flow_probes_and_refs(fc):
        q = rows(pr.q, dtype)
        kp, vp = rows(pr.k[::C, :S0], dtype), rows(pr.v[::C, :S0], dtype)
        kc, vc = rows(pr.k[:, S0:], dtype), rows(pr.v[:, S0:], dtype)
        o1, l1 = ops.attention_fwd(q, kp, vp, B, H, C * T, S0, hd, key_mask=mask, causal=False, scale=pr.scale, save_lse=True)
        o2, l2 = ops.attention_fwd(q, kc, vc, N, H, T, T, hd, causal=True, scale=pr.scale, save_lse=True)
        out = ops.attention_merge(o1, l1, o2, l2, B, C, T, H, hd, out=torch.empty_like(o2))
        worst = max(worst, ap.check({"o": back(out, N, T, H, hd)}, ref, dtype, ok, pr.exact_zero, what=f"{fc.id} {pr.name}"))
        if fc.masked_prompt is not None:                                                        # that question: the candidate segment itself
            sl = slice(fc.masked_prompt * C * T, (fc.masked_prompt + 1) * C * T)
            assert torch.equal(out[sl], o2[sl])
    print(f"score flow {fc.id}: worst error / bound {worst:.3f}")
    note("score flow", worst)


# ------------------------------------------------------------------------------------------------------------------- partial sums
def _partials(values, bias, seed):
    """float32 [3, B, n] whose slices sum exactly to ``values`` [B, n] - bias: value - bias + noise, -noise, 0."""
    noise = ap._ternary(tuple(values.shape), seed) * 4.0
    part = torch.zeros(3, *values.shape, dtype=torch.float64)
    part[0], part[1] = values - bias + noise, -noise
    assert torch.equal(part.float().double(), part) and torch.equal((part.float().sum(0) + bias.float()).double(), values)
    return part.float()


@pytest.mark.parametrize("case", ap.DECODE_CASES, ids=[c.id for c in ap.DECODE_CASES])
def test_decode_from_qkv_partial_sums_plain(ops, case):
    """attention_decode_splitk: q | k | v partial sums plus a bias of small integers that add up exactly to the probe's query and
    newest K / V row; the row is appended at Sk - 1 bit for bit and nothing else in the caches moves."""
    km, keep, ok, _ = setup(case)
    B, H, Sk, hd = case.B, case.H, case.Sk, case.hd
    E, Smax = H * hd, Sk + 9
    bias = torch.randint(-3, 4, (3 * E,), generator=torch.Generator().manual_seed(43)).double()
    assert bool(bias[:E].any() and bias[E:2 * E].any() and bias[2 * E:].any())
    worst = 0.0
    for pr, ref in probes_and_refs(case, False):
        what = f"{case.id} {pr.name}"
        full = torch.cat([pr.q[:, 0].reshape(B, E), pr.k[:, Sk - 1].reshape(B, E), pr.v[:, Sk - 1].reshape(B, E)], 1)
        part = _partials(full, bias, 42)
        kc, vc = _cache(pr.k, Smax), _cache(pr.v, Smax)
        want_k, want_v = kc.clone(), vc.clone()
        kc.view(B, Smax, E)[:, Sk - 1] = -GARBAGE
        vc.view(B, Smax, E)[:, Sk - 1] = -GARBAGE
        o = ops.attention_decode_splitk(part.to(DEV), bias.float().to(DEV), kc, vc, B, H, Sk, hd, kv_batch_rows=Smax,
                                        key_mask=_padded_mask(km, B, Smax), ld_mask=Smax, scale=pr.scale)
        worst = max(worst, ap.check({"o": back(o, B, 1, H, hd)}, ref, BF16, ok, pr.exact_zero, what=what))
        assert torch.equal(kc, want_k) and torch.equal(vc, want_v), what                       # appended at Sk - 1, nothing else touched
    print(f"decode from partial sums, plain {case.id}: worst error / bound {worst:.3f}")
    note("decode from partial sums, plain", worst)


@pytest.mark.parametrize("with_bias", [True, False], ids=["table", "no-table"])
@pytest.mark.parametrize("case", ap.DECODE_REL_CASES, ids=[c.id for c in ap.DECODE_REL_CASES])
def test_decode_from_q_partial_sums_cross(ops, case, with_bias):
    """attention_decode_splitk_rel with part_cols = H hd (cross-attention): the query alone comes from partial sums, K / V are read
    and never written - once with the one-sided bias table, once without a table."""
    km, keep, ok, bias = setup(case)
    B, H, Sk, hd = case.B, case.H, case.Sk, case.hd
    E, Smax = H * hd, Sk + 2
    table, zero = ap.rel_table(case)
    if with_bias:
        todo = probes_and_refs(case, False)                                                     # Probe A: the softmax of the table
    else:                                                                                       # the same case without a table: Probes A and B
        plain = ap.Case(case.B, case.H, 1, case.Sk, case.hd, True, case.mask, note="cross-attention without a table")
        todo = [(pr, ap.reference(pr.q, pr.k, pr.v, None, keep, None, pr.scale)) for pr in ap.probes(plain, keep, ok, False)]
    worst = 0.0
    for pr, ref in todo:
        part = _partials(pr.q[:, 0].reshape(B, E), torch.zeros(E, dtype=torch.float64), 44)
        kc, vc = _cache(pr.k, Smax), _cache(pr.v, Smax)
        want_k, want_v = kc.clone(), vc.clone()
        o = ops.attention_decode_splitk_rel(part.to(DEV), kc, vc, B, H, Sk, hd, kv_batch_rows=Smax, key_mask=_padded_mask(km, B, Smax), scale=pr.scale,
                                            rel_bias=table.to(DEV) if with_bias else None, rel_zero=zero if with_bias else 0)
        worst = max(worst, ap.check({"o": back(o, B, 1, H, hd)}, ref, BF16, ok, pr.exact_zero, what=f"{case.id} {pr.name}"))
        assert torch.equal(kc, want_k) and torch.equal(vc, want_v)                              # nothing appended
    print(f"decode from partial sums, cross {case.id} {'table' if with_bias else 'no table'}: worst error / bound {worst:.3f}")
    note("decode from partial sums, cross", worst)
