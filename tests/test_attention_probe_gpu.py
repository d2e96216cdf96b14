"""GPU: the attention kernels against the exact per-key probes of tests/_attention_probe.py.

Every (query, key) pair shows up on its own in some output element, forward and through each gradient, with right padding, left
padding and holes in the key mask, with and without T5's relative-position bias, at the smallest shapes that reach each kernel
variant (the case tables in _attention_probe.py say which).  One acceptance check, derived from bf16 rounding, serves every probe:
|got - want| <= 2^-8 (abs_companion + |want|) + 1e-6 (1e-5 in fp32), invisible keys read exactly zero, lse within 1e-3.  Each test
prints its worst error / bound; tests/test_attention_probe_cpu.py shows that a kernel wrong by one key would not pass."""
import pytest
import torch

import _attention_probe as ap

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
WORST = {}                                      # kernel family -> worst error / bound seen


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    yield _ops
    print("\nworst error / bound per kernel family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


_SETUP, _REFS = {}, {}


def setup(case):
    """(key mask, visible set, checked rows, bias matrix) of a case, built once."""
    if case not in _SETUP:
        km = ap.key_mask(case)
        keep = ap.visible(case, km)
        _SETUP[case] = (km, keep, ap.rows_checked(case, keep), ap.bias_matrix(case))
    return _SETUP[case]


def probes_and_refs(case, backward):
    """[(probe, float64 reference)] of a case: computed once, shared by every dtype and kernel path, never written to."""
    if (case, backward) not in _REFS:
        km, keep, ok, bias = setup(case)
        _REFS[case, backward] = [(pr, ap.reference(pr.q, pr.k, pr.v, pr.do, keep, bias, pr.scale)) for pr in ap.probes(case, keep, ok, backward)]
    return _REFS[case, backward]


def rows(x, dtype, sel=None):
    """[B, S, H, hd] float64 -> device rows [B S, H hd] (``sel`` bool [B, S]: the packed rows only)."""
    B, S, H, hd = x.shape
    x = x.reshape(B * S, H * hd)
    return (x if sel is None else x[sel.reshape(-1)]).to(dtype).to(DEV).contiguous()


def back(y, B, S, H, hd, sel=None):
    """device rows -> [B, S, H, hd] float64 on the CPU (rows a packed layout does not hold stay zero)."""
    y = y.double().cpu()
    if sel is not None:
        full = torch.zeros(B * S, H * hd, dtype=torch.float64)
        full[sel.reshape(-1)] = y
        y = full
    return y.reshape(B, S, H, hd)


def run_tiled(ops, case, pr, dtype, path=0, rel=False):
    """One probe through attention_fwd (+ attention_bwd), or the _rel pair with the case's bias table: what the kernels returned."""
    km, keep, ok, _ = setup(case)
    B, H, Sq, Sk, hd = case.B, case.H, case.Sq, case.Sk, case.hd
    sel = cu = None
    kw = dict(causal=case.causal, scale=pr.scale)
    if case.lens is not None:
        sel = torch.arange(Sq)[None] < torch.tensor(case.lens)[:, None]
        cu = torch.tensor([0] + list(torch.tensor(case.lens).cumsum(0)), dtype=torch.int32).to(DEV)
        kw["cu_seqlens"] = cu
    else:
        kw["key_mask"] = km.to(DEV) if km is not None else None
    fwd, bwd = ops.attention_fwd, ops.attention_bwd
    if rel:
        table, zero = ap.rel_table(case)
        kw.update(rel_bias=table.to(DEV), rel_zero=zero)
        fwd, bwd = ops.attention_fwd_rel, ops.attention_bwd_rel
    Q, K, V = rows(pr.q, dtype, sel), rows(pr.k, dtype, sel), rows(pr.v, dtype, sel)
    got = {}
    ops.KernelSelect.attention = path
    try:
        o, lse = fwd(Q, K, V, B, H, Sq, Sk, hd, save_lse=True, **kw)
        if pr.do is not None:
            grads = bwd(Q, K, V, o, rows(pr.do, dtype, sel), lse, B, H, Sq, Sk, hd, **kw)
            got.update({n: back(g, B, Sk if n != "dq" else Sq, H, hd, sel) for n, g in zip(("dq", "dk", "dv"), grads)})
    finally:
        ops.KernelSelect.attention = 0
    got["o"], got["lse"] = back(o, B, Sq, H, hd, sel), lse.double().cpu()
    return got


def run_case(ops, family, case, dtype, path=0, rel=False, backward=True):
    km, keep, ok, _ = setup(case)
    worst = 0.0
    for pr, ref in probes_and_refs(case, backward):
        got = run_tiled(ops, case, pr, dtype, path, rel)
        worst = max(worst, ap.check(got, ref, dtype, ok, pr.exact_zero, what=f"{case.id} {pr.name}"))
    print(f"{family} {case.id}: worst error / bound {worst:.3f}")
    WORST[family] = max(WORST.get(family, 0.0), worst)


# ------------------------------------------------------------------------------------------------------------------- plain route
def _plain_params():
    out = []
    for n, c in enumerate(ap.PLAIN_CASES):
        if c.hd == 200:                                         # wide one-tile kernels: bf16 only, no vector-ALU form
            out.append((c, BF16, 0, "wide"))
            continue
        if c.hd == 16:                                          # vector-ALU kernels only
            out += [(c, BF16, 0, "valu bf16"), (c, F32, 0, "valu fp32")]
            continue
        out += [(c, BF16, 0, "mfma"), (c, BF16, 2, "mfma split backward"), (c, BF16, 1, "valu bf16"), (c, F32, 0, "valu fp32")]
        if n == 0:
            out.append((c, BF16, 4, "mfma padded one-tile backward"))
    return out


@pytest.mark.parametrize("case,dtype,path,family", _plain_params(),
                         ids=[f"{c.id}-{'bf16' if d == BF16 else 'fp32'}-path{p}" for c, d, p, _ in _plain_params()])
def test_plain_route(ops, case, dtype, path, family):
    """attention_fwd / attention_bwd: Probes A and B, forward and through dQ, dK and dV."""
    run_case(ops, family, case, dtype, path)


@pytest.mark.parametrize("case", ap.RESIDENT_CASES, ids=[c.id for c in ap.RESIDENT_CASES])
def test_resident_forward_counts_every_key_once(ops, case):
    """fwd_resident64_kernel (path 8): every P entry reads 1 / N."""
    pr, ref = probes_and_refs(case, False)[0]
    assert bool((ref.p == 1.0 / case.Sk).all())
    run_case(ops, "resident forward", case, BF16, 8, backward=False)


# ------------------------------------------------------------------------------------------------------------------- rel route
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", ap.REL_CASES, ids=[c.id for c in ap.REL_CASES])
def test_rel_route(ops, case, dtype):
    """attention_fwd_rel / attention_bwd_rel: Probe A reads the softmax of the bias table out, Probe B selects with the table added."""
    run_case(ops, "rel bf16" if dtype == BF16 else "rel fp32", case, dtype, rel=True)


# ------------------------------------------------------------------------------------------------------------------- packed rows
@pytest.mark.parametrize("case,path", [(ap.PACKED_CASES[0], 0), (ap.PACKED_CASES[1], 0), (ap.PACKED_CASES[1], 4)],
                         ids=lambda v: v.id if isinstance(v, ap.Case) else f"path{v}")
def test_packed_rows(ops, case, path):
    """cu_seqlens, causal, hd 64: per sample, rows of other samples never visible."""
    run_case(ops, "packed rows" + (" padded backward" if path == 4 else ""), case, BF16, path)


# ------------------------------------------------------------------------------------------------------------------- decode step
GARBAGE = 3.0                                   # what the cache rows past Sk hold: finite, and wrong if read


def _cache(x, Smax):
    """[B, Sk, H, hd] -> bf16 device rows [B Smax, H hd] with GARBAGE behind the Sk live rows."""
    B, Sk, H, hd = x.shape
    c = torch.full((B, Smax, H * hd), GARBAGE, dtype=torch.float64)
    c[:, :Sk] = x.reshape(B, Sk, H * hd)
    return c.to(BF16).to(DEV).view(B * Smax, H * hd)


def _padded_mask(km, B, Smax):
    m = torch.zeros(B, Smax, dtype=torch.int32)
    if km is None:
        return None
    m[:, :km.shape[1]] = km
    return m.to(DEV)


@pytest.mark.parametrize("path", [0, 16, 32])
@pytest.mark.parametrize("case", ap.DECODE_CASES, ids=[c.id for c in ap.DECODE_CASES])
def test_decode_step(ops, case, path):
    """attention_fwd with Sq = 1 against a strided cache (every decode kernel variant), and on path 0 the appending attention_decode."""
    km, keep, ok, _ = setup(case)
    B, H, Sk, hd = case.B, case.H, case.Sk, case.hd
    E, Smax = H * hd, Sk + 9
    worst = worst_append = 0.0
    for pr, ref in probes_and_refs(case, False):
        what = f"{case.id} path {path} {pr.name}"
        if pr.name.startswith("B"):
            assert bool(((ref.p == 1.0) | (ref.p < 1e-27)).all()), what                          # one-hot
        q, kc, vc, mask = rows(pr.q, BF16), _cache(pr.k, Smax), _cache(pr.v, Smax), _padded_mask(km, B, Smax)
        ops.KernelSelect.attention = path
        try:
            o, lse = ops.attention_fwd(q, kc, vc, B, H, 1, Sk, hd, key_mask=mask, ld_mask=Smax, causal=True, scale=pr.scale,
                                       kv_batch_rows=Smax, save_lse=True)
        finally:
            ops.KernelSelect.attention = 0
        got = {"o": back(o, B, 1, H, hd), "lse": lse.double().cpu()}
        worst = max(worst, ap.check(got, ref, BF16, ok, pr.exact_zero, what=what))
        if path == 0:
            k_new, v_new = rows(pr.k[:, Sk - 1:], BF16), rows(pr.v[:, Sk - 1:], BF16)
            kc2, vc2 = kc.clone(), vc.clone()
            kc2.view(B, Smax, E)[:, Sk - 1] = -GARBAGE
            vc2.view(B, Smax, E)[:, Sk - 1] = -GARBAGE
            o2 = ops.attention_decode(q, kc2, vc2, k_new, v_new, B, H, Sk, hd, kv_batch_rows=Smax, key_mask=mask, ld_mask=Smax, scale=pr.scale)
            worst_append = max(worst_append, ap.check({"o": back(o2, B, 1, H, hd)}, ref, BF16, ok, pr.exact_zero, what=what + " (appending)"))
            assert torch.equal(kc2, kc) and torch.equal(vc2, vc), what                           # appended at Sk - 1, nothing else touched
    print(f"decode path {path} {case.id}: worst error / bound {worst:.3f}" + (f", appending {worst_append:.3f}" if path == 0 else ""))
    WORST[f"decode path {path}"] = max(WORST.get(f"decode path {path}", 0.0), worst)
    if path == 0:
        WORST["decode appending"] = max(WORST.get("decode appending", 0.0), worst_append)


@pytest.mark.parametrize("case", ap.DECODE_REL_CASES, ids=[c.id for c in ap.DECODE_REL_CASES])
def test_decode_from_partial_sums_with_bias_against_float64(ops, case):
    """attention_decode_splitk_rel, self-attention form: q | k | v partial sums (q columns zero, k | v columns summing exactly to the
    appended indicator row), one-sided bias table: Probe A reads the softmax of the bias out."""
    km, keep, ok, bias = setup(case)
    B, H, Sk, hd = case.B, case.H, case.Sk, case.hd
    E, Smax, ks = H * hd, Sk + 2, 3
    table, zero = ap.rel_table(case)
    worst = 0.0
    for pr, ref in probes_and_refs(case, False):
        new = torch.cat([pr.k[:, Sk - 1].reshape(B, E), pr.v[:, Sk - 1].reshape(B, E)], 1)      # [B, 2 E], bf16 values
        noise = ap._ternary((B, 2 * E), 41) * 4.0                                               # new + noise, -noise, 0: an exact float32 sum
        part = torch.zeros(ks, B, 3 * E, dtype=torch.float64)
        part[0, :, E:], part[1, :, E:] = new + noise, -noise
        assert torch.equal(part.float().double(), part) and torch.equal(part.float().sum(0)[:, E:].double(), new) and not part[:, :, :E].any()
        kc, vc = _cache(pr.k, Smax), _cache(pr.v, Smax)
        want_k, want_v = kc.clone(), vc.clone()
        kc.view(B, Smax, E)[:, Sk - 1] = -GARBAGE
        vc.view(B, Smax, E)[:, Sk - 1] = -GARBAGE
        o = ops.attention_decode_splitk_rel(part.float().to(DEV), kc, vc, B, H, Sk, hd, kv_batch_rows=Smax, key_mask=_padded_mask(km, B, Smax),
                                            scale=pr.scale, rel_bias=table.to(DEV), rel_zero=zero)
        worst = max(worst, ap.check({"o": back(o, B, 1, H, hd)}, ref, BF16, ok, pr.exact_zero, what=f"{case.id} {pr.name}"))
        assert torch.equal(kc, want_k) and torch.equal(vc, want_v)
    print(f"decode from partial sums {case.id}: worst error / bound {worst:.3f}")
    WORST["decode from partial sums, bias"] = max(WORST.get("decode from partial sums, bias", 0.0), worst)
