"""GPU: eavqa_rope, eavqa_rope_finish and eavqa_swiglu_fwd / _bwd / _splitk (csrc/llama.hip) on the probes of tests/_llama_probe.py.

Every case is ONE call of the C entry point through _lib_llama.call, so that every leading dimension is the case's own, on windows into
flat buffers: NaN in the pads of inputs and tables, the sentinel in output pads and in a guard row before and after.  The rope cases
are exact (equality with the float64 reference, first difference reported as (row, column)); the SwiGLU cases are held element by
element to the bound derived in the docstring of _llama_probe.  The multi-pass cases run the grid-stride loops of rope_kernel,
swiglu_fwd_kernel and swiglu_bwd_kernel through three passes with a ragged tail.  tests/test_llama_probe_cpu.py shows, without a GPU,
that the acceptance functions used here reject the address, stride, pass and formula defects these cases exist for.

Worst error / bound of the SwiGLU entry points over all cases, measured on an MI355X: in the docstring of test_swiglu_probes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _llama_probe as P

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


def _call(name, *args):
    from eavqa_amd import _lib_llama
    _lib_llama.call(name, *args)


def _back(dev_backing, view):
    b = dev_backing.cpu()
    return b, b.as_strided(tuple(view.shape), view.stride(), view.storage_offset())


def _dt(ops, dtype: str):
    return ops.dtype_id(P.DT[dtype])


def run_rope(ops, c: P.RopeCase, want=None):
    win, v = P.materialize_rope(c)
    want = P.reference_rope(c, v) if want is None else want
    dev = {nm: P.on_device(b, vw, DEV) for nm, (b, vw) in win.items()}
    pos = v["pos"].to(DEV)
    _call("eavqa_rope", _dt(ops, c.dtype), c.rows, c.H, c.hd, dev["x"][1].data_ptr(), c.ldx, pos.data_ptr(), dev["cos"][1].data_ptr(),
          dev["sin"][1].data_ptr(), c.ld_table, P.N_POS, int(c.inverse), ops._stream())
    P.check_rope(c, want, *_back(dev["x"][0], win["x"][1]))


def run_finish(ops, c: P.FinishCase):
    win, v = P.materialize_finish(c)
    want = P.reference_finish(c, v)
    dev = {nm: P.on_device(b, vw, DEV) for nm, (b, vw) in win.items()}
    pos = v["pos"].to(DEV)
    _call("eavqa_rope_finish", _dt(ops, c.out), c.M, c.H, c.hd, dev["part"][1].data_ptr(), c.ks, pos.data_ptr(), dev["cos"][1].data_ptr(),
          dev["sin"][1].data_ptr(), c.ld_table, P.N_POS, dev["out"][1].data_ptr(), c.ld_out, ops._stream())
    P.check_rope(c, want, *_back(dev["out"][0], win["out"][1]), what="out")


def run_swiglu(ops, c: P.SwigluCase, ref=None):
    win, v = P.materialize_swiglu(c)
    ref = P.reference_swiglu(c, v) if ref is None else ref
    dev = {nm: P.on_device(b, vw, DEV) for nm, (b, vw) in win.items()}
    ptr = lambda nm: dev[nm][1].data_ptr()
    if c.kind == "fwd":
        _call("eavqa_swiglu_fwd", _dt(ops, c.dtype), c.rows, c.F, ptr("u"), c.ldu, ptr("out"), c.ldh, ops._stream())
    elif c.kind == "bwd":
        _call("eavqa_swiglu_bwd", _dt(ops, c.dtype), c.rows, c.F, ptr("u"), c.ldu, ptr("dh"), c.ldh, ptr("out"), c.lddu, ops._stream())
    else:
        _call("eavqa_swiglu_splitk", _dt(ops, c.dtype), c.rows, c.F, ptr("part"), c.ks, ptr("out"), c.ldh, ops._stream())
    P.check_swiglu(c, ref, *_back(dev["out"][0], win["out"][1]))


def _all(run, ops, cases):
    assert cases
    failed = []
    for c in cases:
        try:
            run(ops, c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("dtype,hd", [(d, hd) for d, hds in P.ROPE_HD.items() for hd in hds])
def test_rope_probes(ops, dtype, hd):
    """One head size of one instantiation (float32; bfloat16 with 16-byte items, hd % 16 == 0; bfloat16 with 8-byte items, hd % 16 == 8,
    up to five items a head): H 1 / 3 / 6, 1 / 5 / 67 rows, ldx > H hd, the three table strides, forward and inverse, positions packed,
    repeated, at both ends of the table and out of range on both sides - equality, pads and guard rows untouched."""
    _all(run_rope, ops, [c for c in P.ROPE_CASES if (c.dtype, c.hd) == (dtype, hd) and not c.multipass])


@pytest.mark.parametrize("name", [c.name for c in P.ROPE_CASES if c.multipass])
def test_rope_beyond_the_first_grid_stride_pass(ops, name):
    """Three passes of 524 288 items, the last a ragged tail inside the last row, no pass boundary on a row boundary, skipped rows in both
    full passes: a wrong stride rotates items twice (in place!), a dropped tail or a skipped pass leaves them unrotated.
    f32 vec4: 2053 rows x 511 heads of 8 = 1 049 083 items; bf16 vec8: 2053 x 511 heads of 16 = 1 049 083; bf16 vec4: 2057 rows x 170
    heads of 24 (3 items a head) = 1 049 070."""
    run_rope(ops, P.BY_NAME[name])


@pytest.mark.parametrize("H,hd", [(3, 8), (2, 24), (2, 64), (1, 128)])
def test_rope_finish_probes(ops, H, hd):
    """ks 1 / 3 / 4 slices with a pattern of their own each, M 1 / 33 / 64, both output types, ld_out > 3 H hd with pads and guard rows,
    ld_table > hd / 2: the slice sums exact, q and k rotated, out-of-range rows summed and not rotated, v the plain sum - equality."""
    _all(run_finish, ops, [c for c in P.FINISH_CASES if (c.H, c.hd) == (H, hd)])


@pytest.mark.parametrize("kind", ["fwd", "bwd", "splitk"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_swiglu_probes(ops, kind, dtype):
    """F 4 / 32 / 160 / 2052, 1 / 5 / 65 rows, every leading dimension padded on its own (bwd: ldu != lddu != 2F, lddh != F), guard rows,
    gates over [-30, 30], and the edge table (+-0, the zero of silu', +-16, +-87, +-89, +-104, +- the largest finite value): every
    element inside the derived bound, finite, linear / vanishing beyond the tabled range.
    Worst error / bound measured on an MI355X over these and the multi-pass cases: eavqa_swiglu_fwd 0.226 (float32) / 0.989 (bfloat16),
    eavqa_swiglu_bwd 0.226 / 0.987, eavqa_swiglu_splitk 0.226 / 0.989.  A bfloat16 output's own rounding (2^-8 of the result) is nearly
    the whole of its bound, and some element always comes within about 1 % of half a unit in the last place."""
    _all(run_swiglu, ops, [c for c in P.SWIGLU_CASES if (c.kind, c.dtype) == (kind, dtype) and not c.multipass])
    print("worst error / bound so far:", {" ".join(k): round(x, 4) for k, x in sorted(P.WORST.items())})


@pytest.fixture(scope="module")
def multipass_swiglu_references():
    """kind -> float64 reference of the multi-pass shape: the values are exact in both types, so the two types share it."""
    return {}


@pytest.mark.parametrize("name", [c.name for c in P.SWIGLU_CASES if c.multipass])
def test_swiglu_beyond_the_first_grid_stride_pass(ops, name, multipass_swiglu_references):
    """1027 rows x F = 4100: 1 052 675 items of 4 columns, three passes with a tail of 4099 items (no multiple of 256)."""
    c = P.BY_NAME[name]
    if c.kind not in multipass_swiglu_references:
        multipass_swiglu_references[c.kind] = P.reference_swiglu(c, dict(zip("gbd", P.swiglu_values(c))))
    run_swiglu(ops, c, multipass_swiglu_references[c.kind])
    print("worst error / bound so far:", {" ".join(k): round(x, 4) for k, x in sorted(P.WORST.items())})


# ------------------------------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_swiglu_entry_points_refuse_a_base_one_element_off(ops, dtype):
    """include/eavqa_llama.h: u, h, dh, du aligned to 4 elements, partials to 16 bytes, else EAVQA_E_ALIGN before any launch.  Real
    device allocations, each operand in turn moved by ONE element (every call stays inside its allocation); the outputs keep the
    sentinel, so nothing ran.  bfloat16 moved by 4 elements (8 bytes, not 16) is inside the contract and computes the same values."""
    from eavqa_amd import _lib, _lib_llama
    lib = _lib_llama.load()
    T, es, dt = P.DT[dtype], (4 if dtype == "f32" else 2), _dt(ops, dtype)
    rows, F = 5, 32
    ldu, ldh = 2 * F + 8, F + 8
    u = torch.ones(rows * ldu + 8, dtype=T, device=DEV)
    dh = torch.ones(rows * ldh + 8, dtype=T, device=DEV)
    part = torch.ones(2 * rows * 2 * F + 8, dtype=torch.float32, device=DEV)
    h = torch.full((rows * ldh + 8,), P.SENTINEL, dtype=T, device=DEV)
    du = torch.full((rows * ldu + 8,), P.SENTINEL, dtype=T, device=DEV)
    s = ops._stream()
    p = lambda t, off=0: t.data_ptr() + off * t.element_size()
    E = _lib.EAVQA_E_ALIGN
    assert lib.eavqa_swiglu_fwd(dt, rows, F, p(u), ldu, p(h), ldh, s) == 0
    torch.cuda.synchronize()
    good = h.clone()
    h.fill_(P.SENTINEL)
    assert lib.eavqa_swiglu_fwd(dt, rows, F, p(u, 1), ldu, p(h), ldh, s) == E
    assert lib.eavqa_swiglu_fwd(dt, rows, F, p(u), ldu, p(h, 1), ldh, s) == E
    assert lib.eavqa_swiglu_bwd(dt, rows, F, p(u, 1), ldu, p(dh), ldh, p(du), ldu, s) == E
    assert lib.eavqa_swiglu_bwd(dt, rows, F, p(u), ldu, p(dh, 1), ldh, p(du), ldu, s) == E
    assert lib.eavqa_swiglu_bwd(dt, rows, F, p(u), ldu, p(dh), ldh, p(du, 1), ldu, s) == E
    assert lib.eavqa_swiglu_splitk(dt, rows, F, p(part, 1), 2, p(h), ldh, s) == E
    assert lib.eavqa_swiglu_splitk(dt, rows, F, p(part, 2), 2, p(h), ldh, s) == E              # 8 bytes: partial sums need 16
    assert lib.eavqa_swiglu_splitk(dt, rows, F, p(part), 2, p(h, 1), ldh, s) == E
    torch.cuda.synchronize()
    assert bool((h == P.SENTINEL).all()) and bool((du == P.SENTINEL).all())
    if dtype == "bf16":
        assert lib.eavqa_swiglu_fwd(dt, rows, F, p(u, 4), ldu, p(h, 4), ldh, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(h[4:], good[:-4]) and bool((h[:4] == P.SENTINEL).all())
    else:
        assert lib.eavqa_swiglu_fwd(dt, rows, F, p(u, 2), ldu, p(h), ldh, s) == E              # float32: 8 bytes are not enough


# --------------------------------------------------------------------------------------------------- the wrappers and real strides
def _agrees_or_raises(fn_sliced, fn_dense):
    from eavqa_amd import _lib
    want = fn_dense()
    try:
        got = fn_sliced()
    except _lib.EavqaError:
        return
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want.cpu()), "a column-sliced input was read with the wrong row stride"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_wrappers_pass_the_real_stride_of_a_column_sliced_input(ops, dtype):
    """ops.rope / rope_finish / swiglu_* on views into wider buffers: either the result is the contiguous call's, bit for bit, or the
    wrapper raises - never the values of other rows."""
    T = P.DT[dtype]
    rows, H, hd, F, ks, pad = 7, 2, 16, 32, 3, 8
    val = lambda r, c, m, seed: ((torch.arange(r)[:, None] * 3 + torch.arange(c)[None, :] * 5 + seed) % m - m // 2).float()
    cos_w, sin_w = [t.float().to(DEV) for t in P.table_values(P.N_POS, hd // 2 + pad)]
    cos, sin = cos_w[:, :hd // 2], sin_w[:, :hd // 2]
    pos = P.positions(rows, "mixed").to(DEV)
    # rope: x, and both tables, sliced
    xw = val(rows, H * hd + 2 * pad, 17, 1).to(T).to(DEV)
    _agrees_or_raises(lambda: ops.rope(xw.clone()[:, pad:pad + H * hd], H, hd, pos, cos, sin).contiguous(),
                      lambda: ops.rope(xw[:, pad:pad + H * hd].contiguous(), H, hd, pos, cos.contiguous(), sin.contiguous()))
    # ... and a sin table with another row stride than cos has
    _agrees_or_raises(lambda: ops.rope(xw[:, :H * hd].contiguous(), H, hd, pos, cos, sin.contiguous()),
                      lambda: ops.rope(xw[:, :H * hd].contiguous(), H, hd, pos, cos.contiguous(), sin.contiguous()))
    # rope_finish: partial sums sliced out of wider rows; a sliced output
    E3 = 3 * H * hd
    pw = torch.stack([val(rows, E3 + pad, 5, s) for s in range(ks)]).to(DEV)
    dense = lambda: ops.rope_finish(pw[:, :, :E3].contiguous(), H, hd, pos, cos.contiguous(), sin.contiguous(), T)
    _agrees_or_raises(lambda: ops.rope_finish(pw[:, :, :E3], H, hd, pos, cos.contiguous(), sin.contiguous(), T), dense)
    _agrees_or_raises(lambda: ops.rope_finish(pw[:, :, :E3].contiguous(), H, hd, pos, cos, sin, T), dense)
    ow = torch.full((rows, E3 + pad), P.SENTINEL, dtype=T, device=DEV)
    _agrees_or_raises(lambda: ops.rope_finish(pw[:, :, :E3].contiguous(), H, hd, pos, cos.contiguous(), sin.contiguous(), T, out=ow[:, :E3]).contiguous(), dense)
    assert bool((ow[:, E3:] == P.SENTINEL).all())
    # swiglu: gate | up and dh as slices of wider rows
    uw = (val(rows, 2 * F + 2 * pad, 41, 2) / 4).to(T).to(DEV)
    dw = (val(rows, F + 2 * pad, 9, 3) / 4).to(T).to(DEV)
    u, d = uw[:, pad:pad + 2 * F], dw[:, pad:pad + F]
    _agrees_or_raises(lambda: ops.swiglu_fwd(u), lambda: ops.swiglu_fwd(u.contiguous()))
    _agrees_or_raises(lambda: ops.swiglu_bwd(u, d), lambda: ops.swiglu_bwd(u.contiguous(), d.contiguous()))
    _agrees_or_raises(lambda: ops.swiglu_bwd(u.contiguous(), d), lambda: ops.swiglu_bwd(u.contiguous(), d.contiguous()))
    sw = torch.stack([val(rows, 2 * F + pad, 9, s) / 4 for s in range(ks)]).to(DEV)
    _agrees_or_raises(lambda: ops.swiglu_splitk(sw[:, :, :2 * F], T), lambda: ops.swiglu_splitk(sw[:, :, :2 * F].contiguous(), T))
