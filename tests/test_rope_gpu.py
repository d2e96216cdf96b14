"""GPU: eavqa_rope and eavqa_rope_finish (csrc/llama.hip) against float64 computed from the same float32 cos / sin table.

Bound.  An output is a c -+ b s: two float32 products, one float32 sum and, for bfloat16, one rounding; |c|, |s| <= 1.  Each product
carries a relative error of 2^-24 and the sum another 2^-24 of a result no larger than |a| + |b|, so |err| <= 2^-22 (|a| + |b|) in
float32 with room to spare; the bfloat16 rounding adds 2^-9 of the result, so |err| <= 2^-8 (|a| + |b|)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = {torch.float32: 2.0 ** -22, torch.bfloat16: 2.0 ** -8}
N_POS = 97


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


def table(hd):
    from eavqa_amd.models.lm import rope_table
    return rope_table(N_POS, hd, 10000.0)


def positions(rows, seed):
    """Packed, non-monotonic positions: several restarts, the last table row, and zeros."""
    p = torch.randint(0, N_POS, (rows,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    p[0] = N_POS - 1
    if rows > 1:
        p[1] = 0
    if rows > 4:
        p[2], p[3], p[4] = 5, 3, 0
    return p


def rotate64(x, H, hd, pos, cos, sin, inverse=False):
    """float64 rotation of the first H * hd columns of ``x`` [rows, >= H hd] (a copy); also |a| + |b| per rotated element."""
    rows, half = x.shape[0], hd // 2
    y = x.double().clone()
    v = y[:, :H * hd].reshape(rows, H, hd)
    a, b = v[..., :half].clone(), v[..., half:].clone()
    c, s = cos[pos.long()].double()[:, None, :], sin[pos.long()].double()[:, None, :]
    if inverse:
        s = -s
    out = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    mag = torch.cat([a.abs() + b.abs()] * 2, dim=-1)
    y[:, :H * hd] = out.reshape(rows, H * hd)
    return y, mag.reshape(rows, H * hd)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows", [1, 5, 67])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("hd", [8, 64, 128])
def test_rope_forward_inverse_and_untouched_bytes(ops, dtype, rows, H, hd):
    """q | k columns of QKV-like rows (ldx = 3 H hd + 8): the rotated columns within the bound; the V columns, the pad and every row at
    position 0 bit-unchanged; inverse(forward(x)) within twice the bound."""
    cos, sin = table(hd)
    E, ld = H * hd, 3 * H * hd + 8
    x = rnd(rows, ld, seed=rows + H + hd, dtype=dtype)
    pos = positions(rows, seed=hd + rows)
    d = x.to(DEV).clone()
    ops.rope(d, 2 * H, hd, pos.to(DEV), cos.to(DEV), sin.to(DEV))
    got = d.cpu()
    want, mag = rotate64(x, 2 * H, hd, pos, cos, sin)
    err = (got.double() - want)[:, :2 * E].abs()
    assert bool((err <= EPS[dtype] * mag).all()), (err / mag.clamp_min(1e-30)).max().item()
    assert torch.equal(got[:, 2 * E:], x[:, 2 * E:])                       # V and the pad
    assert torch.equal(got[pos == 0], x[pos == 0])                         # cos = 1, sin = 0
    assert not torch.equal(got[0, :2 * E], x[0, :2 * E])                   # ... and position n_pos - 1 did turn
    ops.rope(d, 2 * H, hd, pos.to(DEV), cos.to(DEV), sin.to(DEV), inverse=True)
    back = (d.cpu().double() - x.double())[:, :2 * E].abs()
    assert bool((back <= 2 * EPS[dtype] * mag).all())
    inv, _ = rotate64(x, 2 * H, hd, pos, cos, sin, inverse=True)           # the inverse on its own is the transposed rotation
    d2 = x.to(DEV).clone()
    ops.rope(d2, 2 * H, hd, pos.to(DEV), cos.to(DEV), sin.to(DEV), inverse=True)
    assert bool(((d2.cpu().double() - inv)[:, :2 * E].abs() <= EPS[dtype] * mag).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_out_of_range_position_leaves_the_row_alone(ops, dtype):
    """Documented in include/eavqa.h: a row whose pos is outside [0, n_pos) is NOT rotated.  Rows sit inside a larger guarded buffer:
    nothing outside the called rows changes either."""
    H, hd, rows, guard = 2, 64, 6, 3
    cos, sin = table(hd)
    ld = H * hd
    buf = rnd(rows + 2 * guard, ld, seed=9, dtype=dtype)
    pos = torch.tensor([3, -1, N_POS, 7, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    d = buf.to(DEV).clone()
    ops.rope(d[guard:guard + rows], H, hd, pos.to(DEV), cos.to(DEV), sin.to(DEV))
    got = d.cpu()
    assert torch.equal(got[:guard], buf[:guard]) and torch.equal(got[guard + rows:], buf[guard + rows:])
    inner, x = got[guard:guard + rows], buf[guard:guard + rows]
    bad = torch.tensor([False, True, True, False, True, True])
    assert torch.equal(inner[bad], x[bad])
    want, mag = rotate64(x[~bad], H, hd, pos[~bad], cos, sin)
    assert bool(((inner[~bad].double() - want).abs() <= EPS[dtype] * mag).all())
    assert not torch.equal(inner[~bad], x[~bad])


def test_rope_bad_sizes_are_errors_not_faults():
    from eavqa_amd import _lib, _lib_llama
    lib = _lib_llama.load()
    base = dict(dtype=1, rows=4, H=2, hd=64, x=16, ldx=128, pos=16, cos=16, sin=16, ld_table=32, n_pos=8, inverse=0, stream=None)
    bad = lambda **kw: lib.eavqa_rope(*[dict(base, **kw)[k] for k in _lib_llama.PARAMS["eavqa_rope"]])
    assert bad(hd=12) == _lib.EAVQA_E_SHAPE and bad(hd=264, ldx=1024, ld_table=132) == _lib.EAVQA_E_SHAPE
    assert bad(ldx=64) == _lib.EAVQA_E_SHAPE and bad(ld_table=16) == _lib.EAVQA_E_SHAPE
    assert bad(ldx=132) == _lib.EAVQA_E_ALIGN and bad(x=18) == _lib.EAVQA_E_ALIGN and bad(ld_table=34) == _lib.EAVQA_E_ALIGN
    assert bad(dtype=2) == _lib.EAVQA_E_DTYPE and bad(pos=None) == _lib.EAVQA_E_ARG and bad(n_pos=0) == _lib.EAVQA_E_ARG
    fin = dict(dtype=1, M=4, H=2, hd=64, partials=16, ks=1, pos=16, cos=16, sin=16, ld_table=32, n_pos=8, out=16, ld_out=384, stream=None)
    badf = lambda **kw: lib.eavqa_rope_finish(*[dict(fin, **kw)[k] for k in _lib_llama.PARAMS["eavqa_rope_finish"]])
    assert badf(hd=12) == _lib.EAVQA_E_SHAPE and badf(ld_out=256) == _lib.EAVQA_E_SHAPE and badf(ks=0) == _lib.EAVQA_E_ARG
    assert badf(out=None) == _lib.EAVQA_E_ARG and badf(dtype=7) == _lib.EAVQA_E_DTYPE


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [1, 33, 64])
@pytest.mark.parametrize("ks", [1, 4])
@pytest.mark.parametrize("H,hd", [(3, 8), (2, 64), (1, 128)])
def test_rope_finish(ops, dtype, M, ks, H, hd):
    """Partial sums [ks][M][3E] -> q | k | v: the reference is the sequential float32 sum of the slices, then the float64 rotation of q
    and k (bound as above, around the summed values) - the v columns equal the rounded sum exactly."""
    cos, sin = table(hd)
    E = H * hd
    part = rnd(ks, M, 3 * E, seed=M + ks + hd)
    pos = positions(M, seed=M + 1)
    if M > 5:
        pos[5] = N_POS + 3                                                 # out of range: that row is summed and left unrotated
    acc = part[0].clone()
    for s in range(1, ks):
        acc = acc + part[s]                                                # float32, slice order
    out = ops.rope_finish(part.to(DEV), H, hd, pos.to(DEV), cos.to(DEV), sin.to(DEV), dtype).cpu()
    assert out.dtype == dtype and tuple(out.shape) == (M, 3 * E)
    assert torch.equal(out[:, 2 * E:], acc[:, 2 * E:].to(dtype))
    ok = (pos >= 0) & (pos < N_POS)
    want, mag = rotate64(acc[ok], 2 * H, hd, pos[ok], cos, sin)
    err = (out[ok].double() - want)[:, :2 * E].abs()
    assert bool((err <= EPS[dtype] * mag).all()), (err / mag.clamp_min(1e-30)).max().item()
    assert torch.equal(out[~ok], acc[~ok].to(dtype))
    assert torch.equal(out[pos == 0], acc[pos == 0].to(dtype))
