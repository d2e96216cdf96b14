"""Bit-exact probes of the normalisation kernels (csrc/norm.hip): the case table, the inputs and one runner per entry point.

tests/golden/norm_bits.json holds one SHA-256 per case, recorded on the MI355X from the commit BEFORE the kernels were restated as one
row body per pass (tests/golden/make_golden_norm_bits.py); tests/test_norm_bits_gpu.py recomputes them.  A digest covers the logical
[rows, cols] region of every output of the call, in a fixed order.  Every output is a window (tests/_gemm_probe.py) into a buffer full
of a sentinel, with one guard row; `run` also reports a write outside a window.

Inputs are closed integer formulas of (row, column) divided by a constant - no RNG stream, no CPU arithmetic that could round
differently on another host (`pat`); the saved mean / rstd of the backward cases are formulas too (the kernels do not require them to belong to
x).  Row 0 has a mean far from zero; the row before the zero row (row 1, in the two-row split-K cases row 0) holds -0.0 at every fifth
column; the zero row (row 2 of the row-per-wave cases, row 1 of the split-K cases) is all zero in every input, which reaches the quantiser's scale-of-1 branch wherever beta and bias are absent
(the split-K fp8 form requires beta: its cases without a bias pass a beta of zeros).
"""
import hashlib

import torch

import _gemm_probe as P

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
X_OF_KIND = {1: "f32", 2: "bf16", 3: "f16"}            # x_kind 0: the storage type of the call
FILL_U8 = 0x5A
ROWS = 5                                               # two workgroups of four waves; three waves of the second exit early
WIDTHS_BWD = (8, 260, 516, 1028, 2052)                 # NV = 2, 2 (a second float4 on lane 0 only), 4, 8, 16
WIDTHS_FWD = WIDTHS_BWD + (4100, 8192)                 # NV = 32
SPLITK_ROWS = 2
SPLITK_WIDE_KS = (2, 3)                                # NV = 8 keeps two slices in flight


def pat(rows, cols, a, b, shift, mod, div):
    """((a r + b c + shift) mod `mod` - mod // 2) / (div + 1/8) as float32: one correctly rounded float64 division and one rounding to
    float32, the same on every host.  The divisor is no power of two, so the values fill their mantissas: products and sums of them
    round, and a fused multiply-add differs from a multiply and an add."""
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    return (((a * r + b * c + shift) % mod - mod // 2).double() / (div + 0.125)).float()


def special_rows(t, zero_row, offset=0.0):
    """Row 0 shifted by `offset`, -0.0 at every fifth column of the row before `zero_row`, row `zero_row` all zero."""
    t[0] += offset
    t[zero_row - 1, 2::5] = -0.0
    t[zero_row] = 0.0
    return t


def row_cases():
    """The row-per-wave entry points.  `opt` bits: 1 strided, 2 gamma, 4 beta / dres, 8 stats / lowp_out."""
    cases = []
    def add(entry, cols, dtype, x_kind, opt, rows=ROWS, dparam=0):
        cases.append(dict(entry=entry, rows=rows, cols=cols, dtype=dtype, x_kind=x_kind, opt=opt, dparam=dparam))
    n = 0
    for cols in WIDTHS_FWD:
        for dtype in ("f32", "bf16", "f16"):
            for x_kind in range(4):
                add("layernorm_fwd", cols, dtype, x_kind, 0b1110)
                add("layernorm_fwd", cols, dtype, x_kind, (0b0001, 0b0101, 0b0011, 0b1001)[n % 4])
                n += 1
        for x_kind in (1, 2, 3):
            add("layernorm_fwd_fp8", cols, "bf16", x_kind, 0b1110)
            add("layernorm_fwd_fp8", cols, "bf16", x_kind, (0b0001, 0b0101, 0b0011, 0b1001)[n % 4])
            n += 1
        for dtype in ("f32", "bf16"):
            for x_kind in range(4):
                add("rmsnorm_fwd", cols, dtype, x_kind, 0b1010)
                add("rmsnorm_fwd", cols, dtype, x_kind, 0b0001 if n % 2 else 0b0011)
                n += 1
    for cols in WIDTHS_BWD:
        for opt in (0b1111, 0b0000, 0b0101, 0b1010):
            for dtype, x_f32 in (("f32", 0), ("f32", 1), ("bf16", 0), ("bf16", 1)):
                add("layernorm_bwd", cols, dtype, x_f32, opt)
            for x_f32 in (0, 1):
                add("layernorm_bwd_fp8", cols, "bf16", x_f32, opt & 0b0111)
            for dtype in ("f32", "bf16"):
                for x_kind in range(4):
                    add("rmsnorm_bwd", cols, dtype, x_kind, opt)
    # dgamma / dbeta onto zeroed buffers: at most two atomics land per column (rows <= 128), and a + b does not depend on the order
    for rows in (5, 70):
        for dtype, x_f32 in (("f32", 1), ("bf16", 0), ("bf16", 1)):
            add("layernorm_bwd", 260, dtype, x_f32, 0b0110, rows=rows, dparam=3)
        add("layernorm_bwd", 260, "bf16", 0, 0b0001, rows=rows, dparam=1)
        add("layernorm_bwd", 260, "bf16", 1, 0b0010, rows=rows, dparam=2)
    return cases


def splitk_cases():
    """The workgroup-per-row entry points.  `opt` bits: 1 strided, 2 bias, 4 x_out."""
    cases = []
    n = 0
    for cols in P.LN_COLS:
        for ks in P.LN_KS + (SPLITK_WIDE_KS if cols > 8192 else ()):
            for entry, dtype in (("layernorm_splitk", "f32"), ("layernorm_splitk", "bf16"), ("layernorm_splitk_fp8", "bf16"),
                                 ("rmsnorm_splitk", "f32"), ("rmsnorm_splitk", "bf16")):
                cases.append(dict(entry=entry, rows=SPLITK_ROWS, cols=cols, dtype=dtype, ks=ks, opt=(0b111, 0b000, 0b011, 0b100, 0b101, 0b010)[n % 6]))
                n += 1
    return cases


def name_of(c):
    return "-".join(f"{k}={c[k]}" for k in ("entry", "rows", "cols", "dtype", "x_kind", "ks", "opt", "dparam") if k in c)


CASES = {name_of(c): c for c in row_cases() + splitk_cases()}
ENTRIES = tuple(dict.fromkeys(c["entry"] for c in CASES.values()))


class _Call:
    """The windows of one call: inputs hold NaN around their data, outputs the sentinel."""

    def __init__(self, dev):
        self.dev, self.outs = dev, []

    def inp(self, values, dtype, ld):
        rows, cols = values.shape
        bk, vw = P.window(rows, cols, ld, DT[dtype], fill=P.NAN)
        vw.copy_(values)
        return P.on_device(bk, vw, self.dev)[1]

    def vec(self, values):
        return self.inp(values.reshape(1, -1), "f32", values.numel())

    def out(self, name, rows, cols, dtype, ld, zero=False):
        fill = FILL_U8 if dtype == "u8" else P.SENTINEL
        bk, vw = P.window(rows, cols, ld, torch.uint8 if dtype == "u8" else DT[dtype], fill=fill)
        if zero:
            vw.zero_()
        b, v = P.on_device(bk, vw, self.dev)
        self.outs.append((name, b, v, fill))
        return v

    def finish(self):
        """(sha256 over the logical region of every output, names of the outputs with a write outside their window)."""
        h, bad = hashlib.sha256(), []
        for name, b, v, fill in self.outs:
            bk = b.cpu()
            vw = bk.as_strided(tuple(v.shape), v.stride(), v.storage_offset())
            h.update(name.encode())
            h.update(P._bits(vw.contiguous()).numpy().tobytes())
            if not P.untouched(bk, vw, fill):
                bad.append(name)
        return h.hexdigest(), bad


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dtype_id(dt):
    from eavqa_amd import _lib
    return _lib.CONSTANTS["EAVQA_" + dt.upper()]


def _run_row(c, call, stream, k):
    rows, cols, opt = c["rows"], c["cols"], c["opt"]
    entry, fwd, rms = c["entry"], "fwd" in c["entry"], c["entry"].startswith("rms")
    fp8 = entry.endswith("fp8")
    ld = cols + 4 if opt & 1 else cols
    dt = c["dtype"]
    xdt = X_OF_KIND.get(c["x_kind"], dt) if (fwd or rms) else ("f32" if (c["x_kind"] or dt == "f32") else dt)
    x = k.inp(special_rows(pat(rows, cols, 37, 11, cols, 257, 32.0), 2, 64.0), xdt, ld)
    gamma = k.vec(1.0 + pat(1, cols, 0, 7, 3, 33, 64.0)) if opt & 2 else None
    dtype_id = _dtype_id(dt)
    if fwd:
        beta = k.vec(pat(1, cols, 0, 5, 1, 17, 32.0)) if (opt & 4 and not rms) else None
        y = k.out("yq" if fp8 else "y", rows, cols, "u8" if fp8 else dt, ld)
        scale = k.out("scale", 1, rows, "f32", rows) if fp8 else None
        mean = k.out("mean", 1, rows, "f32", rows) if (opt & 8 and not rms) else None
        rstd = k.out("rstd", 1, rows, "f32", rows) if opt & 8 else None
        if rms:
            call("eavqa_rmsnorm_fwd", dtype_id, c["x_kind"], rows, cols, _ptr(x), ld, _ptr(gamma), 1e-6, _ptr(y), ld, _ptr(rstd), stream)
        elif fp8:
            call("eavqa_layernorm_fwd_fp8", c["x_kind"], rows, cols, _ptr(x), ld, _ptr(gamma), _ptr(beta), 1e-5, _ptr(y), ld, _ptr(scale),
                 _ptr(mean), _ptr(rstd), stream)
        else:
            call("eavqa_layernorm_fwd", dtype_id, c["x_kind"], rows, cols, _ptr(x), ld, _ptr(gamma), _ptr(beta), 1e-5, _ptr(y), ld,
                 _ptr(mean), _ptr(rstd), stream)
        return
    r = torch.arange(rows)
    mean = k.vec((((3 * r + 1) % 7 - 3).double() / 8.0 + 64.0 * (r == 0)).float())
    rstd = k.vec(torch.tensor([1.0, 0.5, 0.25, 2.0, 0.125])[r % 5])
    dy = k.inp(special_rows(pat(rows, cols, 29, 13, cols + 1, 129, 64.0), 2), dt, ld)
    dres = k.inp(special_rows(pat(rows, cols, 17, 7, cols + 2, 65, 16.0), 2), "f32", ld) if opt & 4 else None
    dx = k.out("dx", rows, cols, "f32", ld)
    lowp = k.out("dx_lowp", rows, cols, dt, ld) if (opt & 8 and not fp8) else None
    if rms:
        call("eavqa_rmsnorm_bwd", dtype_id, c["x_kind"], rows, cols, _ptr(x), ld, _ptr(dy), ld, _ptr(gamma), _ptr(rstd), _ptr(dres), _ptr(dx), ld,
             _ptr(lowp), ld if lowp is not None else 0, stream)
    elif fp8:
        dxq, scale = k.out("dxq", rows, cols, "u8", ld), k.out("scale", 1, rows, "f32", rows)
        call("eavqa_layernorm_bwd_fp8", c["x_kind"], rows, cols, _ptr(x), ld, _ptr(dy), ld, _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dres),
             _ptr(dx), ld, _ptr(dxq), ld, _ptr(scale), stream)
    else:
        dgamma = k.out("dgamma", 1, cols, "f32", cols, zero=True) if c["dparam"] & 1 else None
        dbeta = k.out("dbeta", 1, cols, "f32", cols, zero=True) if c["dparam"] & 2 else None
        call("eavqa_layernorm_bwd", dtype_id, c["x_kind"], rows, cols, _ptr(x), ld, _ptr(dy), ld, _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dres),
             _ptr(dx), ld, _ptr(dgamma), _ptr(dbeta), _ptr(lowp), ld if lowp is not None else 0, stream)


def _run_splitk(c, call, stream, k):
    rows, cols, ks, opt, entry = c["rows"], c["cols"], c["ks"], c["opt"], c["entry"]
    pad = 4 if opt & 1 else 0
    fp8, rms = entry.endswith("fp8"), entry.startswith("rms")
    with_bias = bool(opt & 2) and not rms
    x = k.inp(special_rows(pat(rows, cols, 37, 11, cols, 257, 32.0), 1, 64.0), "f32", cols + pad)
    part = None
    if ks:
        p = pat(ks * rows, cols, 19, 3, cols + ks, 129, 64.0)
        p[1::rows] = 0.0                                                # the zero row of every slice
        part = k.inp(p, "f32", cols)
    bias = k.vec(pat(1, cols, 0, 9, 2, 9, 8.0)) if with_bias else None
    gamma = k.vec(1.0 + pat(1, cols, 0, 7, 3, 33, 64.0))
    beta = k.vec(torch.zeros(1, cols) if (fp8 and not with_bias) else pat(1, cols, 0, 5, 1, 17, 32.0))
    x_out = k.out("x_out", rows, cols, "f32", cols + 2 * pad) if opt & 4 else None
    y = k.out("yq" if fp8 else "y", rows, cols, "u8" if fp8 else c["dtype"], cols + 3 * pad)
    ld_out = cols + 2 * pad if x_out is not None else 0
    dtype_id = _dtype_id(c["dtype"])
    if rms:
        call("eavqa_rmsnorm_splitk", dtype_id, rows, cols, _ptr(x), cols + pad, _ptr(part), ks, _ptr(x_out), ld_out, _ptr(gamma), 1e-6,
             _ptr(y), cols + 3 * pad, stream)
    elif fp8:
        scale = k.out("scale", 1, rows, "f32", rows)
        call("eavqa_layernorm_splitk_fp8", rows, cols, _ptr(x), cols + pad, _ptr(part), ks, _ptr(bias), _ptr(x_out), ld_out, _ptr(gamma),
             _ptr(beta), 1e-5, _ptr(y), cols + 3 * pad, _ptr(scale), stream)
    else:
        call("eavqa_layernorm_splitk", dtype_id, rows, cols, _ptr(x), cols + pad, _ptr(part), ks, _ptr(bias), _ptr(x_out), ld_out, _ptr(gamma),
             _ptr(beta), 1e-5, _ptr(y), cols + 3 * pad, stream)


def run(c, call, stream, dev="cuda"):
    """One case through `call(name, *args)` (eavqa_amd._lib.call): (digest, outputs written outside their window)."""
    k = _Call(dev)
    (_run_splitk if "ks" in c else _run_row)(c, call, stream, k)
    torch.cuda.synchronize()
    return k.finish()
