"""Exact probes of the GEMM family: windows into flat buffers, integer data, one float64 reference, the case tables (no GPU needed here).

Why integers: with operands from {-2..2} every product sum is an integer far below 2^24, so it is exact in fp32 in ANY summation order -
the expectation of a kernel's result is `torch.equal` with the float64 reference, not a bound.  Why windows: every matrix of a call is a
[rows, cols] view with row stride `ld` into one flat backing buffer whose remaining elements hold NaN (inputs: a kernel that reads one
of them turns its result into NaN) or a finite sentinel (outputs: a kernel that writes one of them is caught by `untouched`).

tests/test_gemm_probe_cpu.py asserts, without a GPU, that every case below is exact, is routed to the kernel it names, that the tables
cover what they claim, and that `check` / `check_splitk` / `check_finish` / `check_decode` - the functions the GPU tests use - reject
twelve one-line mutations of a plain emulation of the kernels.
"""
import zlib
from dataclasses import dataclass, field, replace
from typing import Optional, Tuple

import numpy as np
import torch

F32, GEN, SKINNY, FAST, SHAPED, BIG, K64 = range(7)             # Kind, as include/eavqa_test.h numbers it
KIND_NAMES = {F32: "f32general", GEN: "general", SKINNY: "skinny", FAST: "fast", SHAPED: "shaped", BIG: "big", K64: "k64"}
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "fp8": torch.uint8}
NAN = float("nan")
NAN_E4M3 = 0x7F                 # the NaN byte of OCP e4m3
SENTINEL = -24832.0             # -97 * 2^8: finite, exact in bf16 / half / float32, outside every range a case may store
LIMIT = {"bf16": 256.0, "f16": 2048.0, "f32": float(2 ** 24)}          # integers every format below holds exactly
NO_ROW_SPLIT = 1 << 25


# ------------------------------------------------------------------------------------------------------------------------ windows
def window(rows: int, cols: int, ld: int, dtype: torch.dtype, *, elem_offset: int = 0, guard_rows: int = 1, fill):
    """(backing, view): a flat buffer full of `fill` and a [rows, cols] view of it with row stride `ld`, `elem_offset` elements in.
    `ld - cols` guard columns follow every row and `guard_rows` whole rows follow the last one."""
    if rows <= 0 or cols <= 0 or elem_offset < 0 or guard_rows < 0:
        raise ValueError("window: rows, cols > 0 and elem_offset, guard_rows >= 0")
    if ld < cols:
        raise ValueError(f"window: row stride {ld} < {cols} columns - the rows of the view would overlap their own guard")
    backing = torch.full((elem_offset + (rows + guard_rows) * ld,), fill, dtype=dtype)
    return backing, backing.as_strided((rows, cols), (ld, 1), elem_offset)


def on_device(backing, view, dev):
    """The same window on `dev` (the flat buffer copied as it is: pads and guards travel with it)."""
    b = backing.to(dev)
    return b, b.as_strided(tuple(view.shape), view.stride(), view.storage_offset())


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def untouched(backing, view, fill=SENTINEL) -> bool:
    """Every element of `backing` outside `view` still holds the bits of `fill`."""
    outside = torch.ones(backing.numel(), dtype=torch.bool)
    outside.as_strided(tuple(view.shape), view.stride(), view.storage_offset()).fill_(False)
    want = _bits(torch.full((1,), fill, dtype=backing.dtype))
    return bool((_bits(backing.cpu())[outside] == want).all())


def c4(n: int) -> int:
    return (n + 3) // 4 * 4


# --------------------------------------------------------------------------------------------------------------------------- data
def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ints(g, shape, lo: int, hi: int, step: int = 1):
    return (torch.randint(0, (hi - lo) // step + 1, shape, generator=g) * step + lo).double()


def residual_of(M: int, N: int):
    """An integer function of (m, n) with different periods along the two axes: a swapped row or column changes it."""
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return ((3 * m + 5 * n) % 17 - 8).double()


def operand_values(g, vals: str, M: int, N: int, K: int):
    """A [M, K], B [N, K] as float64 integers.  pm2: {-2..2}; pm1: {-1, 0, 1} (large K, alpha = 2); half: B even (alpha = 0.5 keeps
    integers), half1: the same with A from {-1, 0, 1}; small: two +-1 per row of A, B even - |alpha A B^T| <= 2 at alpha = 0.5 (the non-linear activations)."""
    if vals == "pm2":
        return ints(g, (M, K), -2, 2), ints(g, (N, K), -2, 2)
    if vals == "pm1":
        return ints(g, (M, K), -1, 1), ints(g, (N, K), -1, 1)
    if vals == "half":
        return ints(g, (M, K), -2, 2), ints(g, (N, K), -2, 2, 2)
    if vals == "half1":
        return ints(g, (M, K), -1, 1), ints(g, (N, K), -2, 2, 2)
    if vals == "small":
        a = torch.zeros(M, K, dtype=torch.float64)
        cols = torch.stack([torch.randperm(K, generator=g)[:2] for _ in range(M)])
        a.scatter_(1, cols, ints(g, (M, 2), -1, 1, 2))
        return a, ints(g, (N, K), -2, 2, 2)
    raise ValueError(vals)


def to_storage(x, dtype: str):
    """float64 integers -> the storage type (e4m3 as bytes)."""
    if dtype == "fp8":
        return x.float().to(torch.float8_e4m3fn).view(torch.uint8)
    return x.to(DT[dtype])


def from_storage(t, dtype: str):
    if dtype == "fp8":
        return t.view(torch.float8_e4m3fn).double()
    return t.double()


ACT_F = {
    "none": lambda x: x, "relu": lambda x: x.clamp_min(0), "tanh": torch.tanh,
    "gelu_new": lambda x: 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3))),
    "quick_gelu": lambda x: x * torch.sigmoid(1.702 * x),
}


def act_grad(act: str, u):
    if act == "none":
        return torch.ones_like(u)
    if act == "relu":
        return (u > 0).double()
    uu = u.clone().requires_grad_(True)
    ACT_F[act](uu).sum().backward()
    return uu.grad


EXACT_ACTS = ("none", "relu")
NONLINEAR = ("tanh", "gelu_new", "quick_gelu")


def act_tol(dtype: str, scale: float) -> float:
    """`tol(dtype, scale)` of tests/test_ops_gpu.py: 2e-5 (float32 operands) / 2e-2 (bf16 operands) times scale."""
    return (2e-5 if dtype == "f32" else 2e-2) * scale


# -------------------------------------------------------------------------------------------------------------- tiled GEMM cases
@dataclass(frozen=True)
class GemmCase:
    name: str
    tile: str                       # key of TILES (the kernel the case means to hit); fp8: "fp8.<i>"
    kind: int                       # what eavqa_gemm_route must report for (dtype, layouts, M, N, K, knobs) ...
    index: int
    split: int                      # ... and its split_rows
    knobs: int
    dtype: str                      # operands: bf16 | f32 | fp8
    a_kc: bool
    b_kc: bool
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    out: str = "f32"                # f32 | bf16 | f16
    ldc: int = 0
    c_off: int = 0
    aux: Optional[str] = None       # None | "out" | "in"
    ld_aux: int = 0
    aux_off: int = 0
    res: Optional[str] = None       # None | f32 | bf16 | f16 | "inplace" (residual = the output window)
    ldr: int = 0
    res_off: int = 0
    bias: Optional[int] = None      # element offset of the bias vector in its buffer (0: 16-byte aligned), None: no bias
    act: str = "none"
    alpha: float = 1.0
    vals: str = "pm2"
    aspects: Tuple[str, ...] = ()
    prefetch: bool = False
    fp8_tile: int = 0               # eavqa_gemm_fp8's `tile` argument (1-based entry of FP8_SHAPES)

    @property
    def res_dtype(self):
        return self.out if self.res == "inplace" else self.res

    def vec_flags(self):
        """(vec_c, vec_aux, vec_res, vec_bias) as fill_params (csrc/gemm.hip) derives them from a 16-byte aligned backing buffer."""
        esz = 4 if self.dtype == "f32" else 2
        def ok(off, ld, es):
            return (off * es) % (4 * es) == 0 and ld % 4 == 0
        vc = ok(self.c_off, self.ldc, 4 if self.out == "f32" else esz)
        va = ok(self.aux_off, self.ld_aux, esz) if self.aux else True
        if self.res == "inplace":
            vr = vc
        else:
            vr = ok(self.res_off, self.ldr, 4 if self.res == "f32" else esz) if self.res else True
        vb = (self.bias * 4) % 16 == 0 if self.bias is not None else True
        return vc, va, vr, vb


# name -> (kind, index, knobs, tile rows, tile columns, k per step, stages of the kernel's ring).  The geometry is the kernel's own table
# entry: K64_SHAPES (csrc/gemm_k64.hip: launch_k64s<WM, WN, MF, NF, NST, LW>, 16 MF WM x 16 NF WN, BK = 64), SHAPES and the 128 x 128 /
# 256 x 256 kernels of csrc/gemm_r1.hip (BK = 32, four stages; 256 x 256: BK = 64, two), the double-buffered general kernels.
TILES = {
    "fast": (FAST, 0, (1 << 18) | (1 << 8), 128, 128, 32, 4),
    "big": (BIG, 0, (2 << 14) | NO_ROW_SPLIT, 256, 256, 64, 2),
    "skinny": (SKINNY, 0, 0, 64, 16, 32, 8),
}
for _i, (_bm, _bn) in enumerate([(128, 80), (128, 96), (256, 128), (256, 160), (256, 192)]):
    TILES[f"shaped.{_i}"] = (SHAPED, _i, (_i + 2) << 18, _bm, _bn, 32, 4)
for _i, (_bm, _bn, _st) in enumerate([(128, 80, 3), (128, 80, 3), (128, 128, 2), (256, 128, 3), (256, 160, 3), (128, 80, 4), (128, 96, 3),
                                      (256, 192, 2), (256, 256, 2), (128, 128, 3), (128, 256, 3)]):
    TILES[f"k64.{_i}"] = (K64, _i, (_i + 2) << 8, _bm, _bn, 64, _st)
for _l in range(4):
    TILES[f"general.{_l}"] = (GEN, _l, (1 << 7) if _l == 0 else 0, 128, 128, 64, 2)
    TILES[f"f32general.{_l}"] = (F32, _l, 0, 128, 128, 16, 2)
FP8_TILES = [(128, 80, 4), (256, 128, 3), (256, 160, 3), (128, 128, 3), (128, 256, 3)]          # FP8_SHAPES (csrc/gemm_fp8.hip), BK = 128


def _validates(c: GemmCase) -> bool:
    """validate() of csrc/gemm.hip on the case's shape and leading dimensions (the backing buffers are 16-byte aligned)."""
    vec = 16 if c.dtype == "fp8" else 8 if c.dtype == "bf16" else 4
    a_contig, b_contig = (c.K if c.a_kc else c.M), (c.K if c.b_kc else c.N)
    if a_contig % vec or b_contig % vec or (c.dtype == "fp8" and c.K % 128):
        return False
    if c.lda % vec or c.ldb % vec or c.lda < a_contig or c.ldb < b_contig or c.ldc < c.N:
        return False
    if c.aux and c.ld_aux < c.N:
        return False
    if c.res and c.res != "inplace" and c.ldr < c.N:
        return False
    if c.dtype == "f32" and (c.out != "f32" or c.res_dtype not in (None, "f32")):
        return False                      # 16-bit streams: bf16 operands only
    if "f16" in (c.out, c.res_dtype) and (c.out not in ("f16", "f32") or c.res_dtype not in (None, "f16", "f32")):
        return False                      # a half stream: half (or float32) for both the residual and the output
    if c.dtype == "fp8" and (c.out == "f16" or c.res_dtype not in (None, "f32")):
        return False                      # eavqa_gemm_fp8: C bf16 or float32, a float32 residual
    return True


def _family(tile: str, dtype: str, a_kc: bool, b_kc: bool, M: int, N: int, K1: int, Kdeep: int, *, split: int = 0, knobs=None, order: int = 0,
            fp8_tile: int = 0, lean: bool = False):
    """The aspects of the issue on one kernel: strided operands, guards, the four alignment flags one at a time and together, in place,
    head layout.  K1: one k-step; Kdeep: one more k-step than the ring has stages."""
    if fp8_tile:
        kind, index, kn = -1, fp8_tile - 1, 0
    else:
        kind, index, kn = TILES[tile][:3]
    kn = kn if knobs is None else knobs
    vec = 16 if dtype == "fp8" else 8 if dtype == "bf16" else 4
    lowp = dtype == "bf16"
    sixteen = ("bf16", "f16")[order % 2] if lowp else "f32"
    cyc = lambda i: ("f32", "bf16", "f16")[(order + i) % 3] if lowp else "f32"
    n4 = c4(N)

    def mk(tag, K, aspects, **kw):
        a_c, b_c = (K if a_kc else M), (K if b_kc else N)
        strided = "strided" in aspects
        base = dict(name=f"{tile}-{dtype}-{M}x{N}-{tag}", tile=tile, kind=kind, index=index, split=split, knobs=kn, dtype=dtype, a_kc=a_kc, b_kc=b_kc,
                    M=M, N=N, K=K, lda=a_c + (vec if strided else 0), ldb=b_c + ((2 * vec if b_kc else vec) if strided else 0), ldc=n4,
                    aspects=tuple(aspects), fp8_tile=fp8_tile, vals="half1" if dtype == "fp8" else "pm2")
        base.update(kw)
        if base.get("aux") and not base.get("ld_aux"):
            base["ld_aux"] = n4
        if base.get("res") and base["res"] != "inplace" and not base.get("ldr"):
            base["ldr"] = n4
        return GemmCase(**base)

    deep_vals = "half1" if dtype == "fp8" else "pm1"
    cases = [
        mk("strided", K1, ["strided"]),
        mk("strided+guards", Kdeep, ["strided", "guards"], vals=deep_vals, ldc=n4 + 8, aux="out", ld_aux=n4 + 24, res="f32", ldr=n4 + 16, bias=0,
           act="relu"),
    ]
    if lean:
        return [c for c in cases if _validates(c)]
    res16 = "f32" if dtype == "fp8" else None
    cases += [
        # each flag 0 on its own (an element off 16-byte alignment, or a row stride that is no multiple of 4), the others 1
        mk("vec_c=0", K1, ["align", "vec_c"], out=cyc(1), ldc=n4, c_off=1, aux="out", res=res16 or cyc(1), bias=0, act="relu"),
        mk("vec_aux=0", K1, ["align", "vec_aux", "aux_in"], out=cyc(0), aux="in", ld_aux=n4 + 9, res=res16 or cyc(0), bias=0, act="relu"),
        mk("vec_res=0", K1, ["align", "vec_res"], out=cyc(2), aux="out", res=res16 or cyc(2), ldr=n4 + 4, res_off=1, bias=0),
        mk("vec_bias=0", K1, ["align", "vec_bias"], out=cyc(0), aux="out", res=res16 or cyc(0), bias=1, act="relu"),
        mk("vec_all=0", K1, ["align", "vec_c", "vec_aux", "vec_res", "vec_bias"], out=cyc(1), ldc=n4 + 5, c_off=1, aux="out", ld_aux=n4 + 9, aux_off=3,
           res=res16 or cyc(1), ldr=n4 + 13, res_off=1, bias=3, act="relu"),
        # the head: out = buf[:, :N], the row stride a multiple of 4 and the base aligned - vector stores are allowed up to the ragged edge
        mk("head", K1, ["head"], out="f32", ldc=n4 + 4, alpha=2.0, vals="half1" if dtype == "fp8" else "pm1", bias=0),
        mk("head16", K1, ["head"], out="bf16" if dtype != "f32" else "f32", ldc=n4 + 8, alpha=2.0 if dtype == "fp8" else 0.5, vals="half1" if dtype == "fp8" else "half", bias=0),
    ]
    if dtype != "fp8":
        cases += [
            # _wgrad's gview and the tower's stream: out and residual are one strided, unaligned window
            mk("inplace", K1, ["inplace"], out="f32", ldc=n4 + 12, c_off=1, res="inplace", bias=0),
            mk("inplace16", K1, ["inplace"], out=sixteen, ldc=n4 + 12, c_off=1, res="inplace", bias=0),
        ]
    return [c for c in cases if _validates(c)]


def _nonlinear(tile: str, dtype: str, M: int, N: int, K: int):
    """The three configurations tests/test_ops_gpu.py bounds (test_gemm_epilogue_forward: float32 output with residual, storage-type
    output; test_gemm_epilogue_activation_backward), on an exact pre-activation of magnitude <= 3, strided and guarded."""
    kind, index, kn = TILES[tile][:3]
    vec = 8 if dtype == "bf16" else 4
    n4 = c4(N)
    out = []
    for act in NONLINEAR:
        base = dict(tile=tile, kind=kind, index=index, split=0, knobs=kn, dtype=dtype, a_kc=True, b_kc=True, M=M, N=N, K=K, lda=K + vec,
                    ldb=K + 2 * vec, vals="small", alpha=0.5, act=act)
        out.append(GemmCase(name=f"{tile}-{dtype}-{M}x{N}-{act}-fwd", out="f32", ldc=n4 + 8, aux="out", ld_aux=n4 + 24, res="f32", ldr=n4 + 16, bias=1,
                            aspects=("nonlinear", "strided", "guards"), **base))
        out.append(GemmCase(name=f"{tile}-{dtype}-{M}x{N}-{act}-fwd-storage", out=dtype, ldc=n4 + 8, bias=0, aspects=("nonlinear", "strided", "guards"),
                            **base))
        out.append(GemmCase(name=f"{tile}-{dtype}-{M}x{N}-{act}-bwd", out="f32", ldc=n4 + 8, aux="in", ld_aux=n4 + 9, aspects=("nonlinear", "strided", "aux_in"),
                            **base))
    return out


def _build_gemm_cases():
    cases = []
    order = 0
    for tile, (kind, index, kn, bm, bn, bk, st) in TILES.items():
        if kind in (F32, GEN):
            continue
        if kind == SKINNY:
            for N in (73, 201):                                  # M <= 64; ragged against the 16 columns of a workgroup; N >= 64
                cases += _family(tile, "bf16", True, True, 37, N, 32, 32 * 11, order=order, lean=N == 73)
            cases += _family(tile, "bf16", True, True, 64, 89, 96, 32 * 17, order=order + 1, lean=True)         # K % 64 != 0: per_wave * 8 > nsteps
        else:
            cases += _family(tile, "bf16", True, True, 2 * bm + 9, 2 * bn + 9, bk, bk * (st + 1), order=order)
        order += 1
    # the 256 x 256 kernel with its ragged last tile row in a second launch (rows_from): the smallest shape whose split saves a round
    cases += _family("big", "bf16", True, True, 16448, 1000, 64, 192, split=64, knobs=2 << 14, lean=True)
    for lay in range(4):
        a_kc, b_kc = lay < 2, lay % 2 == 0
        for dtype, tile, k_odd in (("bf16", f"general.{lay}", 72), ("f32", f"f32general.{lay}", 68)):
            M = 265 if a_kc else 264
            N = 265 if b_kc else 264
            k1 = TILES[tile][5]
            cases += _family(tile, dtype, a_kc, b_kc, M, N, k1, 3 * k1, order=lay)
            cases += _family(tile, dtype, a_kc, b_kc, M, 785 if b_kc else 784, k_odd, k_odd, order=lay + 1)       # K no multiple of 64
    # the default route with a look-ahead region (the PF instantiations of the full-line tiles)
    pf = _family("k64.5", "bf16", True, True, 265, 169, 64, 320, knobs=0, lean=True)[1]
    cases.append(replace(pf, name="pf-" + pf.name, prefetch=True, aspects=pf.aspects + ("prefetch",)))
    for i, (bm, bn, st) in enumerate(FP8_TILES):
        cases += _family(f"fp8.{i}", "fp8", True, True, 2 * bm + 9, 2 * bn + 9, 128, 128 * (st + 1), fp8_tile=i + 1, order=i)
    for tile, dtype, M in (("general.0", "bf16", 150), ("f32general.0", "f32", 150), ("fast", "bf16", 150), ("k64.5", "bf16", 150),
                           ("big", "bf16", 300), ("skinny", "bf16", 40)):
        cases += _nonlinear(tile, dtype, M, 265, 64)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), "case names must be unique"
    return cases


@dataclass
class Bufs:
    """The windows of one case, on the CPU: name -> (backing, view)."""
    win: dict = field(default_factory=dict)
    a_scale: Optional[torch.Tensor] = None
    b_scale: float = 1.0


def materialize(c: GemmCase):
    """(bufs, values): the windows of the case - inputs hold their data with NaN around it, outputs the sentinel - and the float64 values."""
    g = _gen(c.name)
    a, b = operand_values(g, c.vals, c.M, c.N, c.K)
    v = {"a": a, "b": b}
    bufs = Bufs()
    nan = NAN_E4M3 if c.dtype == "fp8" else NAN
    for nm, x, kc, ld in (("a", a, c.a_kc, c.lda), ("b", b, c.b_kc, c.ldb)):
        x = x if kc else x.T
        bk, vw = window(x.shape[0], x.shape[1], ld, DT[c.dtype], fill=nan)
        vw.copy_(to_storage(x, c.dtype))
        bufs.win[nm] = (bk, vw)
    if c.dtype == "fp8":
        bufs.a_scale = torch.tensor([1.0, 0.5])[torch.arange(c.M) % 2].float()       # powers of two; B is even, so every scaled sum is an integer
        bufs.b_scale = 1.0
    aux_dt = "bf16" if c.dtype == "fp8" else c.dtype
    if c.bias is not None:
        v["bias"] = ints(g, (c.N,), -1, 1) if c.vals == "small" else ints(g, (c.N,), -3, 3)
        bk, vw = window(1, c.N, c.N, torch.float32, elem_offset=c.bias, fill=NAN)
        vw.copy_(v["bias"])
        bufs.win["bias"] = (bk, vw)
    if c.aux == "in":
        u = ints(g, (c.M, c.N), -3, 3)
        v["aux_in"] = u
        bk, vw = window(c.M, c.N, c.ld_aux, DT[aux_dt], elem_offset=c.aux_off, fill=NAN)
        vw.copy_(u)
        bufs.win["aux"] = (bk, vw)
    elif c.aux == "out":
        bufs.win["aux"] = window(c.M, c.N, c.ld_aux, DT[aux_dt], elem_offset=c.aux_off, fill=SENTINEL)
    bufs.win["c"] = window(c.M, c.N, c.ldc, DT[c.out], elem_offset=c.c_off, fill=SENTINEL)
    if c.res:
        v["res"] = residual_of(c.M, c.N)
        if c.res == "inplace":
            bufs.win["c"][1].copy_(v["res"])
        else:
            bk, vw = window(c.M, c.N, c.ldr, DT[c.res], elem_offset=c.res_off, fill=NAN)
            vw.copy_(v["res"])
            bufs.win["res"] = (bk, vw)
    return bufs, v


def reference(c: GemmCase, bufs: Bufs, v: dict):
    """float64: {"pre": alpha (row scale) A B^T + bias (what aux_out holds), "c": the output before its rounding to the output type}."""
    acc = v["a"] @ v["b"].T
    scale = c.alpha * bufs.b_scale
    pre = acc * scale
    if bufs.a_scale is not None:
        pre = pre * bufs.a_scale.double()[:, None]
    if c.bias is not None:
        pre = pre + v["bias"][None, :]
    if c.aux == "in":
        out = pre * act_grad(c.act, v["aux_in"])
    else:
        out = ACT_F[c.act](pre)
    if c.res:
        out = out + v["res"]
    return {"pre": pre, "c": out, "abs": (v["a"].abs() @ v["b"].abs().T).max().item()}


WORST = {}          # (operand dtype, configuration) -> worst error / bound of the non-linear cases seen by check()


def check(c: GemmCase, ref: dict, got: Bufs):
    """Raises AssertionError unless the windows in `got` (CPU copies of the buffers after the call) hold what the case expects."""
    cb, cv = got.win["c"]
    assert untouched(cb, cv), f"{c.name}: C was written outside its [M, N] window"
    if c.aux == "out":
        ab, av = got.win["aux"]
        assert untouched(ab, av), f"{c.name}: aux_out was written outside its [M, N] window"
        assert torch.equal(av.double(), ref["pre"]), f"{c.name}: aux_out differs from the exact pre-activation"
    if c.act in EXACT_ACTS:
        assert torch.equal(cv.double(), ref["c"]), f"{c.name}: C differs from the exact result: {_first_diff(cv.double(), ref['c'])}"
        return
    if c.aux == "in":
        conf, bound = "bwd", act_tol(c.dtype, 0.2)
    elif c.out == "f32":
        conf, bound = "fwd", act_tol(c.dtype, 0.1 if c.dtype == "f32" else 1.0)
    else:
        conf, bound = "fwd-storage", act_tol(c.dtype, 2.0)
    err = (cv.double() - ref["c"]).abs().max().item()
    key = (c.dtype, c.act, conf)
    WORST[key] = max(WORST.get(key, 0.0), err / bound)
    assert err <= bound, f"{c.name}: |C - reference| = {err:.3e} > {bound:.3e}"         # (NaN fails too)


def _first_diff(got, want):
    bad = (got != want) | got.isnan()
    if not bad.any():
        return "none"
    i = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} elements, first at {i}: got {got[tuple(i)].item()}, want {want[tuple(i)].item()}"


def exactness_violations(c: GemmCase, ref: dict, v: dict):
    """The invariant of the module docstring for one case; a list of what breaks it (empty: exact)."""
    bad = []
    if not ref["abs"] < 2 ** 24:
        bad.append("sum |a||b| >= 2^24")
    aux_dt = "bf16" if c.dtype == "fp8" else c.dtype
    stored = [("pre", ref["pre"], aux_dt if c.aux == "out" else "f32")]
    if c.act in EXACT_ACTS:
        stored.append(("c", ref["c"], c.out))
    for nm, x, dt in stored:
        if not torch.equal(x, x.round()):
            bad.append(f"{nm} is not integral")
        lim = LIMIT[dt]
        if not (x.abs().max().item() <= lim if dt != "f32" else x.abs().max().item() < lim):
            bad.append(f"|{nm}| = {x.abs().max().item()} beyond what {dt} holds exactly")
        if (x == SENTINEL).any():
            bad.append(f"{nm} produces the sentinel")
    for nm in ("res", "aux_in", "bias"):
        if nm in v and v[nm].abs().max().item() > 256:
            bad.append(f"{nm} beyond 256")
    if c.act in NONLINEAR and ref["pre"].abs().max().item() > 3:
        bad.append("non-linear case with |pre-activation| > 3")
    return bad


# ------------------------------------------------------------------------------------------------- emulation of a GEMM through windows
def _flat(bufs, nm, dtype):
    return from_storage(bufs.win[nm][0], dtype).numpy()


def _geo(bufs, nm):
    vw = bufs.win[nm][1]
    return vw.storage_offset(), vw.stride(0)


def _take(flat, off, ld, rows, cols):
    return np.take(flat, off + rows[:, None] * ld + cols[None, :], mode="clip")


def _put(bufs, nm, off, ld, rows, cols, vals):
    bk = bufs.win[nm][0]
    idx = torch.from_numpy(off + rows[:, None] * ld + cols[None, :]).reshape(-1)
    bk[idx] = torch.from_numpy(np.ascontiguousarray(vals)).reshape(-1).to(bk.dtype)


GEMM_MUTATIONS = ("lda_is_K", "chunk_past_K", "store4_at_ragged_N", "row_M_written", "residual_ldc", "aux_out_ldc", "bias_rounded_down")


def emulate_gemm(c: GemmCase, bufs: Bufs, mutation: Optional[str] = None):
    """eavqa_gemm in plain index arithmetic over the flat buffers (k-contiguous operands, an exact activation); `mutation`: one of
    GEMM_MUTATIONS, the one-line address bug it names.  Writes C and aux_out into `bufs`."""
    assert c.a_kc and c.b_kc and c.act in EXACT_ACTS
    vec = 16 if c.dtype == "fp8" else 8 if c.dtype == "bf16" else 4
    m, n = np.arange(c.M), np.arange(c.N)
    k = np.arange(c.K + (vec if mutation == "chunk_past_K" else 0))
    a_off, lda = _geo(bufs, "a")
    b_off, ldb = _geo(bufs, "b")
    A = _take(_flat(bufs, "a", c.dtype), a_off, c.K if mutation == "lda_is_K" else lda, m, k)
    B = _take(_flat(bufs, "b", c.dtype), b_off, ldb, n, k)
    pre = (A @ B.T) * (c.alpha * bufs.b_scale)
    if bufs.a_scale is not None:
        pre = pre * bufs.a_scale.double().numpy()[:, None]
    if c.bias is not None:
        off = _geo(bufs, "bias")[0]
        pre = pre + np.take(_flat(bufs, "bias", "f32"), (off // 4 * 4 if mutation == "bias_rounded_down" else off) + n, mode="clip")[None, :]
    c_off, ldc = _geo(bufs, "c")
    aux_dt = "bf16" if c.dtype == "fp8" else c.dtype
    out = pre
    if c.aux == "in":
        off, ld = _geo(bufs, "aux")
        u = _take(_flat(bufs, "aux", aux_dt), off, ld, m, n)
        out = pre * (u > 0 if c.act == "relu" else 1.0)
    elif c.act == "relu":
        out = np.maximum(pre, 0)
    if c.res:
        nm = "c" if c.res == "inplace" else "res"
        off, ld = _geo(bufs, nm)
        out = out + _take(_flat(bufs, nm, c.res_dtype), off, ldc if mutation == "residual_ldc" else ld, m, n)
    rows, cols = m, n
    if mutation == "store4_at_ragged_N":
        cols = np.arange(c4(c.N))
    if mutation == "row_M_written":
        rows = np.arange(c.M + 1)
    def widen(x):
        y = np.zeros((len(rows), len(cols)))
        y[:c.M, :c.N] = x
        return y
    if c.aux == "out":
        off, ld = _geo(bufs, "aux")
        _put(bufs, "aux", off, ldc if mutation == "aux_out_ldc" else ld, rows, cols, widen(pre))
    _put(bufs, "c", c_off, ldc, rows, cols, widen(out))


# ------------------------------------------------------------------------------------------------------------------ split-K cases
@dataclass(frozen=True)
class SplitKCase:
    name: str
    fp8: bool
    M: int
    N: int
    ks: int                 # 0: the plan's own value
    nsteps: int             # k-steps of one slice (32 values in bf16, 128 in e4m3)
    U: int                  # depth of the weight-load window the case means to hit
    sel: int                # selector of eavqa_gemm_splitk_ex: [7:0] U, [11:8] waves, [15:12] 16-column fragments per wave; 0: the library's
    lda_pad: int
    ldb_pad: int

    @property
    def step(self):
        return 128 if self.fp8 else 32

    def resolve(self, plan=None):
        """(ks, k-values per slice).  ks = 0: `nsteps` counts the steps of the whole K and `plan` (eavqa_gemm[_fp8]_splitk_plan) cuts it."""
        if self.ks:
            return self.ks, self.nsteps * self.step
        ks = int(plan(self.M, self.N, self.nsteps * self.step))
        assert ks > 0 and self.nsteps % ks == 0
        return ks, self.nsteps * self.step // ks


def splitk_variant(sel: int):
    """(U, NW, NF) as splitk_plan (csrc/decode_params.h) decodes a selector: [7:0] U, [11:8] waves (0: 8), [15:12] 16-column fragments a wave (0: 1)."""
    return sel & 0xFF, ((sel >> 8) & 0xF) or 8, ((sel >> 12) & 0xF) or 1


# every variant eavqa_gemm_splitk_ex instantiates (for each of its three row-fragment counts): NF {1, 2} x NW {4, 8} x U {8, 16}
SPLITK_VARIANTS = tuple((U, NW, NF) for NF in (1, 2) for NW in (4, 8) for U in (8, 16))
SPLITK_SELS = tuple(U | (NW << 8) | (NF << 12) for U, NW, NF in SPLITK_VARIANTS)
SPLITK_MS = (1, 16, 17, 32, 33, 64)


def _build_splitk_cases():
    cases = []
    i = 0
    for sel in SPLITK_SELS:
        U, nw, nf = splitk_variant(sel)
        cols = 16 * nw * nf
        for nsteps in (1, U - 1, U, U + 1, 2 * U + 1):
            M = SPLITK_MS[i % 6]
            ks = (1, 2, 3)[i % 3]
            assert nsteps * 32 * (1 if M <= 16 else 2 if M <= 32 else 4) * 32 <= 150 * 1024              # the staged A slice (splitk_plan)
            cases.append(SplitKCase(f"splitk-{sel:04x}-M{M}-ks{ks}-n{nsteps}", False, M, cols + cols // 2 + 9, ks, nsteps, U, sel, 8, 16))
            i += 1
    # the library's own choice: U = 16 from 512 k-values a slice on, the plan's ks
    for M, nsteps, ks in ((17, 64, 0), (64, 7, 0), (33, 17, 2), (1, 15, 3)):
        cases.append(SplitKCase(f"splitk-auto-M{M}-ks{ks}-n{nsteps}", False, M, 201, ks, nsteps, 16 if (nsteps >= 16 and ks) else 8, 0, 8, 16))
    # e4m3: a k-step is 128 values; U = 8 from 1024 values a slice on, else 4
    for j, (U, nsteps) in enumerate([(4, 1), (4, 3), (4, 4), (4, 5), (8, 8), (8, 9), (8, 17)]):
        M = SPLITK_MS[j % 6]
        assert nsteps * 128 * (1 if M <= 16 else 2 if M <= 32 else 4) * 16 <= 150 * 1024
        cases.append(SplitKCase(f"splitk-fp8-M{M}-ks{(1, 2, 3)[j % 3]}-n{nsteps}", True, M, 201, (1, 2, 3)[j % 3], nsteps, U, 0, 16, 32))
    cases.append(SplitKCase("splitk-fp8-auto-M17-n4", True, 17, 201, 0, 4, 4, 0, 16, 32))
    return cases


def materialize_splitk(c: SplitKCase, ks: int, KS: int):
    g = _gen(c.name)
    K = ks * KS
    a, b = operand_values(g, "half" if c.fp8 else ("pm1" if K > 512 else "pm2"), c.M, c.N, K)
    dt = "fp8" if c.fp8 else "bf16"
    bufs = Bufs()
    for nm, x, pad in (("a", a, c.lda_pad), ("b", b, c.ldb_pad)):
        bk, vw = window(x.shape[0], K, K + pad, DT[dt], fill=NAN_E4M3 if c.fp8 else NAN)
        vw.copy_(to_storage(x, dt))
        bufs.win[nm] = (bk, vw)
    if c.fp8:
        bufs.a_scale = torch.tensor([0.5, 2.0, 1.0])[torch.arange(c.M) % 3].float()       # powers of two whose products with b_scale are integers
        bufs.b_scale = 2.0
    bufs.win["part"] = window(ks * c.M, c.N, c.N, torch.float32, fill=SENTINEL)
    return bufs, {"a": a, "b": b}


def reference_splitk(c: SplitKCase, ks: int, KS: int, bufs: Bufs, v: dict):
    """[ks, M, N]: the product of every slice's own k-range, scales applied."""
    sc = bufs.b_scale * (bufs.a_scale.double()[:, None] if bufs.a_scale is not None else 1.0)
    return torch.stack([(v["a"][:, s * KS:(s + 1) * KS] @ v["b"][:, s * KS:(s + 1) * KS].T) * sc for s in range(ks)])


def check_splitk(c: SplitKCase, ks: int, ref, got: Bufs):
    pb, pv = got.win["part"]
    assert untouched(pb, pv), f"{c.name}: partial sums written outside [ks, M, N]"
    part = pv.double().view(ks, c.M, c.N)
    for s in range(ks):
        assert torch.equal(part[s], ref[s]), f"{c.name}: slice {s} is not the product of its own k-range: {_first_diff(part[s], ref[s])}"
    assert torch.equal(part.sum(0), ref.sum(0)), f"{c.name}: the slices do not add up to the product"


SPLITK_MUTATIONS = ("drops_last_step", "starts_at_previous_k0")


def emulate_splitk(c: SplitKCase, ks: int, KS: int, bufs: Bufs, mutation: Optional[str] = None):
    dt = "fp8" if c.fp8 else "bf16"
    m, n = np.arange(c.M), np.arange(c.N)
    A, B = _flat(bufs, "a", dt), _flat(bufs, "b", dt)
    (a_off, lda), (b_off, ldb) = _geo(bufs, "a"), _geo(bufs, "b")
    sc = bufs.b_scale * (bufs.a_scale.double().numpy()[:, None] if bufs.a_scale is not None else 1.0)
    for s in range(ks):
        k0 = (max(s - 1, 0) if mutation == "starts_at_previous_k0" else s) * KS
        nsteps = KS // c.step
        nsteps -= 1 if (mutation == "drops_last_step" and nsteps % c.U) else 0
        k = k0 + np.arange(nsteps * c.step)
        p = (_take(A, a_off, lda, m, k) @ _take(B, b_off, ldb, n, k).T) * sc
        _put(bufs, "part", 0, c.N, s * c.M + m, n, p)


# ------------------------------------------------------------------------------------------------------------------- finish cases
@dataclass(frozen=True)
class FinishCase:
    name: str
    gated: bool
    M: int
    N: int                          # columns of the result (gated: F; the partial sums have 2 F)
    ks: int
    n_seg: int
    out: str                        # f32 | bf16
    lds: Tuple[int, ...]            # row stride of every destination segment (the last one of n_seg = 3: a K/V-cache row, S_max * E)
    act: str
    bias: bool
    ldr: int                        # 0: no residual


FINISH_KS = (1, 2, 7, 8, 9)
ACTS = ("none", "relu") + NONLINEAR


def _build_finish_cases():
    cases = []
    i = 0
    for n_seg in (1, 2, 3):
        for ks in FINISH_KS:
            for out in ("f32", "bf16"):
                act = ACTS[(i + i // 10 * 2) % 5]               # (every ks and output type meets an exact and a non-linear activation)
                M = (5, 17, 33, 64, 1)[i % 5]
                seg = (52, 36, 20)[n_seg - 1]                  # M N / 4 is no multiple of 256 for any M above
                N = seg * n_seg
                lds = tuple([seg + 4, seg + 12, 3 * seg][j] for j in range(n_seg))
                cases.append(FinishCase(f"finish-seg{n_seg}-ks{ks}-{out}-{act}-M{M}", False, M, N, ks, n_seg, out, lds, act, i % 4 != 3,
                                        N + 8 if i % 2 == 0 else 0))
                i += 1
    for ks in FINISH_KS:
        for out in ("f32", "bf16"):
            act = ACTS[i % 5]
            M = (5, 17, 33, 64, 1)[i % 5]
            cases.append(FinishCase(f"finish-gated-ks{ks}-{out}-{act}-M{M}", True, M, 52, ks, 1, out, (60,), act, False, 0))
            i += 1
    return cases


def materialize_finish(c: FinishCase):
    g = _gen(c.name)
    cols = 2 * c.N if c.gated else c.N
    nonlin = c.act in NONLINEAR
    # the sum over slices stays an integer of magnitude <= 3 (non-linear activations: the bound below is absolute) or <= 27
    if nonlin:
        part = torch.zeros(c.ks, c.M, cols, dtype=torch.float64)
        part[torch.randint(0, c.ks, (1,), generator=g).item()] = ints(g, (c.M, cols), -2, 2)
        d = ints(g, (c.M, cols), -3, 3)                   # ... while every slice still matters: +d in the first, -d in the last
        if c.ks > 1:
            part[0] += d
            part[-1] -= d
    else:
        part = ints(g, (c.ks, c.M, cols), -1, 1) if c.gated else ints(g, (c.ks, c.M, cols), -3, 3)
    v = {"part": part}
    bufs = Bufs()
    bk, vw = window(c.ks * c.M, cols, cols, torch.float32, fill=NAN)
    vw.copy_(part.view(c.ks * c.M, cols))
    bufs.win["part"] = (bk, vw)
    if c.bias:
        v["bias"] = ints(g, (c.N,), -1, 1)
        bk, vw = window(1, c.N, c.N, torch.float32, fill=NAN)
        vw.copy_(v["bias"])
        bufs.win["bias"] = (bk, vw)
    if c.ldr:
        v["res"] = residual_of(c.M, c.N)
        bk, vw = window(c.M, c.N, c.ldr, torch.float32, fill=NAN)
        vw.copy_(v["res"])
        bufs.win["res"] = (bk, vw)
    seg = c.N // c.n_seg
    for j in range(c.n_seg):
        bufs.win[f"out{j}"] = window(c.M, seg, c.lds[j], DT[c.out], fill=SENTINEL)
    return bufs, v


def reference_finish(c: FinishCase, v: dict):
    s = v["part"].sum(0)
    if c.gated:
        return ACT_F[c.act](s[:, :c.N]) * s[:, c.N:]
    if c.bias:
        s = s + v["bias"][None, :]
    s = ACT_F[c.act](s)
    return s + v["res"] if c.ldr else s


def finish_bound(c: FinishCase) -> float:
    """Non-linear activations: act_fwd of csrc/common.h is the tiled epilogue's, so its bound is that epilogue's (test_gemm_epilogue_forward:
    float32 values tol(float32, 0.1), a bf16 store tol(bfloat16, 2.0)); the gate multiplies the activation by an integer of magnitude <= 2."""
    return (act_tol("f32", 0.1) if c.out == "f32" else act_tol("bf16", 2.0)) * (2.0 if c.gated else 1.0)


def check_finish(c: FinishCase, ref, got: Bufs):
    seg = c.N // c.n_seg
    for j in range(c.n_seg):
        ob, ov = got.win[f"out{j}"]
        assert untouched(ob, ov), f"{c.name}: segment {j} written outside its window"
        want = ref[:, j * seg:(j + 1) * seg]
        if c.act in EXACT_ACTS:
            assert torch.equal(ov.double(), want), f"{c.name}: segment {j}: {_first_diff(ov.double(), want)}"
        else:
            err = (ov.double() - want).abs().max().item()
            key = ("finish", c.act, c.out)
            WORST[key] = max(WORST.get(key, 0.0), err / finish_bound(c))
            assert err <= finish_bound(c), f"{c.name}: segment {j}: |out - reference| = {err:.3e} > {finish_bound(c):.3e}"


FINISH_MUTATIONS = ("first_8_slices", "boundary_column_to_neighbour")


def emulate_finish(c: FinishCase, bufs: Bufs, mutation: Optional[str] = None):
    assert c.act in EXACT_ACTS
    cols = 2 * c.N if c.gated else c.N
    P = _flat(bufs, "part", "f32").reshape(-1)[:c.ks * c.M * cols].reshape(c.ks, c.M, cols)
    s = P[:min(c.ks, 8) if mutation == "first_8_slices" else c.ks].sum(0)
    m = np.arange(c.M)
    act = (lambda x: np.maximum(x, 0)) if c.act == "relu" else (lambda x: x)
    if c.gated:
        out = act(s[:, :c.N]) * s[:, c.N:]
    else:
        if c.bias:
            s = s + _flat(bufs, "bias", "f32")[:c.N][None, :]
        out = act(s)
        if c.ldr:
            off, ld = _geo(bufs, "res")
            out = out + _take(_flat(bufs, "res", "f32"), off, ld, m, np.arange(c.N))
    seg = c.N // c.n_seg
    for n in range(c.N):
        sg, nl = n // seg, n % seg
        if mutation == "boundary_column_to_neighbour" and nl == 0 and sg > 0:
            sg, nl = sg - 1, seg
        _put(bufs, f"out{sg}", 0, c.lds[sg], m, np.array([nl]), out[:, n:n + 1])


# ------------------------------------------------------------------------------------------------------ direct decode GEMM cases
@dataclass(frozen=True)
class DecodeCase:
    name: str
    M: int
    N: int                          # output columns (gated: F)
    K: int
    sel: int                        # selector of eavqa_gemm_decode_ex (bits [3:0]: forced 16-column fragments, bit 7: rotate)
    gated: bool = False
    bias: bool = False
    act: str = "none"
    out: str = "f32"
    n_seg: int = 1
    residual: bool = False
    want_stats: bool = False


def _build_decode_cases():
    cases = []
    for i, (M, nf) in enumerate([(5, 1), (16, 2), (17, 3), (32, 4), (33, 1), (64, 2), (1, 4), (16, 3)]):
        cols = 16 * nf
        N = 2 * cols + cols // 2 + 3                             # ragged against the workgroup's columns, odd
        cases.append(DecodeCase(f"decode-M{M}-nf{nf}-plain", M, N, 64 * (1 + i % 3) if i % 2 else 64 * 9, nf, bias=i % 2 == 0, act=("none", "relu")[i % 2],
                                out=("f32", "bf16")[i % 2], residual=True, want_stats=True))
    # three segments whose width (40) is no multiple of the workgroup's columns (16 nf), the last two with a cache row's stride
    for M, nf in ((7, 1), (32, 2), (64, 2)):
        cases.append(DecodeCase(f"decode-M{M}-nf{nf}-seg3", M, 120, 192, nf, bias=True, out="bf16", n_seg=3, residual=False))
    cases.append(DecodeCase("decode-M17-nf2-seg3-rot", 17, 120, 64 * 17, 2 | 0x80, bias=True, out="f32", n_seg=3, residual=True, want_stats=True))
    # T5's gate with a bias (bias[gate_rows + n] is a read of its own): NF counts both halves, so it is even
    for M, nf, act in ((5, 2, "relu"), (33, 2, "none"), (32, 4, "relu"), (16, 4, "none")):
        cases.append(DecodeCase(f"decode-M{M}-nf{nf}-gated-{act}", M, 8 * nf * 2 + 5, 128, nf, gated=True, bias=True, act=act, out=("f32", "bf16")[M % 2],
                                residual=M % 2 == 1))
    return cases


def materialize_decode(c: DecodeCase):
    g = _gen(c.name)
    rows_b = 2 * c.N if c.gated else c.N
    vals = "small" if c.gated else "pm1" if c.K > 256 else "pm2"          # (the gate multiplies two sums: both stay below 8)
    a, b = operand_values(g, vals, c.M, rows_b, c.K)
    v = {"a": a, "b": b}
    bufs = Bufs()
    for nm, x, pad in (("a", a, 8), ("b", b, 16)):
        bk, vw = window(x.shape[0], c.K, c.K + pad, torch.bfloat16, fill=NAN)
        vw.copy_(x)
        bufs.win[nm] = (bk, vw)
    if c.bias:
        v["bias"] = ints(g, (rows_b,), -3, 3)
        bk, vw = window(1, rows_b, rows_b, torch.float32, fill=NAN)
        vw.copy_(v["bias"])
        bufs.win["bias"] = (bk, vw)
    if c.residual:
        v["res"] = residual_of(c.M, c.N)
        bk, vw = window(c.M, c.N, c4(c.N) + 12, torch.float32, fill=NAN)
        vw.copy_(v["res"])
        bufs.win["res"] = (bk, vw)
    seg = c.N // c.n_seg
    for j in range(c.n_seg):
        bufs.win[f"out{j}"] = window(c.M, seg, (seg + 3 + 4 * j) if j < 2 else 3 * seg + 1, DT[c.out], fill=SENTINEL)
    return bufs, v


def reference_decode(c: DecodeCase, v: dict):
    s = v["a"] @ v["b"].T
    if c.bias:
        s = s + v["bias"][None, :]
    out = ACT_F[c.act](s[:, :c.N]) * s[:, c.N:] if c.gated else ACT_F[c.act](s)
    return out + v["res"] if c.residual else out


def check_decode(c: DecodeCase, ref, got: Bufs):
    seg = c.N // c.n_seg
    for j in range(c.n_seg):
        ob, ov = got.win[f"out{j}"]
        assert untouched(ob, ov), f"{c.name}: segment {j} written outside its window"
        want = ref[:, j * seg:(j + 1) * seg]
        assert torch.equal(ov.double(), want), f"{c.name}: segment {j}: {_first_diff(ov.double(), want)}"


DECODE_MUTATIONS = ("gated_bias_at_n",)


def emulate_decode(c: DecodeCase, bufs: Bufs, mutation: Optional[str] = None):
    assert c.act in EXACT_ACTS
    m, n, k = np.arange(c.M), np.arange(c.N), np.arange(c.K)
    (a_off, lda), (b_off, ldb) = _geo(bufs, "a"), _geo(bufs, "b")
    A, B = _flat(bufs, "a", "bf16"), _flat(bufs, "b", "bf16")
    bias = _flat(bufs, "bias", "f32") if c.bias else np.zeros(2 * c.N)
    act = (lambda x: np.maximum(x, 0)) if c.act == "relu" else (lambda x: x)
    Am = _take(A, a_off, lda, m, k)
    out = act(Am @ _take(B, b_off, ldb, n, k).T + bias[n][None, :])
    if c.gated:
        gb = bias[n if mutation == "gated_bias_at_n" else c.N + n]
        out = out * (Am @ _take(B, b_off, ldb, c.N + n, k).T + gb[None, :])
    if c.residual:
        off, ld = _geo(bufs, "res")
        out = out + _take(_flat(bufs, "res", "f32"), off, ld, m, n)
    seg = c.N // c.n_seg
    for j in range(c.n_seg):
        off, ld = _geo(bufs, f"out{j}")
        _put(bufs, f"out{j}", off, ld, m, np.arange(seg), out[:, j * seg:(j + 1) * seg])


def range_violations(x, dt: str):
    """What keeps the float64 integers `x` from being stored exactly as `dt` (empty: nothing)."""
    bad = []
    if not torch.equal(x, x.round()):
        bad.append("not integral")
    lim = LIMIT[dt]
    if not x.abs().max().item() <= (lim if dt != "f32" else lim - 1):
        bad.append(f"magnitude {x.abs().max().item()} beyond what {dt} holds exactly")
    if (x == SENTINEL).any():
        bad.append("produces the sentinel")
    return bad


GEMM_CASES = _build_gemm_cases()
SPLITK_CASES = _build_splitk_cases()
FINISH_CASES = _build_finish_cases()
DECODE_CASES = _build_decode_cases()

# ---------------------------------------------------------------------------------------------------- LayerNorm over partial sums
LN_KS = (0, 1, 7, 8, 9, 16, 17)
LN_COLS = (4, 2044, 2048, 2052, 4100, 8200, 16384)      # 512 threads x 4 columns x NV: NV = 1 up to 2048, 2 up to 4096, 4 up to 8192, 8 up to 16384
LN_COLS_REJECTED = 16388
