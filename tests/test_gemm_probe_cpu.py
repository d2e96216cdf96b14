"""CPU: the case tables of tests/_gemm_probe.py are what they claim to be, and the checks the GPU probes use reject wrong kernels.

Exactness: every case keeps the invariant of the probe (integers, sum |a||b| < 2^24, stored magnitudes inside what the destination type
holds exactly), computed here from the float64 reference.  Routing: eavqa_gemm_route (host only) sends every tiled case to the kernel
it names.  Coverage: every (kernel, aspect) pair the tables promise occurs.  Mutations: twelve one-line address / range bugs put into a
plain emulation of the kernels are each rejected by `check` / `check_splitk` / `check_finish` / `check_decode`, while the unmutated
emulation passes.
"""
import copy
import ctypes as C
from collections import Counter

import pytest
import torch

import _gemm_probe as P


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------- windows
def test_window_geometry_and_untouched():
    backing, view = P.window(3, 5, 8, torch.bfloat16, elem_offset=1, guard_rows=1, fill=P.SENTINEL)
    assert backing.numel() == 1 + 4 * 8 and view.shape == (3, 5) and view.stride() == (8, 1) and view.storage_offset() == 1
    assert P.untouched(backing, view)
    view.fill_(7.0)
    assert P.untouched(backing, view)                       # writes inside the window do not count
    for idx in (0, 6, 1 + 2 * 8 + 5, 1 + 3 * 8, backing.numel() - 1):       # before, guard column, behind the last row's columns, guard row, end
        b = backing.clone()
        b[idx] = 0.0
        assert not P.untouched(b, b.as_strided((3, 5), (8, 1), 1)), idx
    b = backing.clone()
    b[0] = -P.SENTINEL                                      # the comparison is on bits
    assert not P.untouched(b, b.as_strided((3, 5), (8, 1), 1))
    nan_b, nan_v = P.window(2, 4, 4, torch.float32, fill=P.NAN)
    assert torch.isnan(nan_b).all() and P.untouched(nan_b, nan_v, fill=P.NAN)


def test_window_rejects_a_view_that_overlaps_its_own_guard():
    with pytest.raises(ValueError):
        P.window(4, 9, 8, torch.float32, fill=0.0)          # row stride below the column count: row r + 1 starts inside row r
    with pytest.raises(ValueError):
        P.window(4, 8, 8, torch.float32, elem_offset=-1, fill=0.0)
    with pytest.raises(ValueError):
        P.window(0, 8, 8, torch.float32, fill=0.0)
    for c in P.GEMM_CASES:                                  # ... and no case asks for one
        assert c.ldc >= c.N and (not c.aux or c.ld_aux >= c.N) and (c.res in (None, "inplace") or c.ldr >= c.N), c.name


# -------------------------------------------------------------------------------------------------------------------- exactness
@pytest.fixture(scope="module")
def gemm_refs():
    """Reference of every tiled / fp8 case, computed once."""
    out = {}
    for c in P.GEMM_CASES:
        bufs, v = P.materialize(c)
        out[c.name] = (bufs, v, P.reference(c, bufs, v))
    return out


def test_every_gemm_case_is_exact(gemm_refs):
    bad = {}
    for c in P.GEMM_CASES:
        bufs, v, ref = gemm_refs[c.name]
        viol = P.exactness_violations(c, ref, v)
        # what the windows hold IS the float64 data (no rounding on the way into bf16 / half / e4m3)
        for nm, key in (("a", "a"), ("b", "b"), ("res", "res"), ("bias", "bias")):
            if nm in bufs.win and key in v:
                x = v[key] if nm not in ("a", "b") or getattr(c, f"{nm}_kc") else v[key].T
                dt = c.dtype if nm in ("a", "b") else (c.res if nm == "res" else "f32")
                if not torch.equal(P.from_storage(bufs.win[nm][1], dt), x.reshape(bufs.win[nm][1].shape)):
                    viol.append(f"{nm} is rounded by its storage type")
        if viol:
            bad[c.name] = viol
    assert not bad, bad


def test_every_decode_family_case_is_exact(lib):
    bad = {}
    for c in P.SPLITK_CASES:
        plan = lib.eavqa_gemm_fp8_splitk_plan if c.fp8 else lib.eavqa_gemm_splitk_plan
        ks, KS = c.resolve(plan)
        bufs, v = P.materialize_splitk(c, ks, KS)
        ref = P.reference_splitk(c, ks, KS, bufs, v)
        viol = [f"slice {s}: {x}" for s in range(ks) for x in P.range_violations(ref[s], "f32")] + P.range_violations(ref.sum(0), "f32")
        if not (v["a"].abs() @ v["b"].abs().T).max().item() < 2 ** 24:
            viol.append("sum |a||b|")
        assert KS % c.step == 0 and (ks * KS) % (c.step * ks) == 0
        if viol:
            bad[c.name] = viol
    for c in P.FINISH_CASES:
        bufs, v = P.materialize_finish(c)
        ref = P.reference_finish(c, v)
        pre = v["part"].sum(0)
        viol = P.range_violations(pre, "f32")
        if c.act in P.EXACT_ACTS:
            viol += P.range_violations(ref, c.out)
        elif pre.abs().max().item() + (1 if c.bias else 0) > 3:
            viol.append("non-linear case with |pre-activation| > 3")
        assert (c.M * c.N // 4) % 256 != 0 and c.N % (4 * c.n_seg) == 0, c.name
        if viol:
            bad[c.name] = viol
    for c in P.DECODE_CASES:
        bufs, v = P.materialize_decode(c)
        viol = P.range_violations(P.reference_decode(c, v), c.out)
        if viol:
            bad[c.name] = viol
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------- routing
def test_every_tiled_case_is_routed_to_the_kernel_it_names(lib):
    wrong = {}
    for c in P.GEMM_CASES:
        if c.dtype == "fp8":
            assert 1 <= c.fp8_tile <= len(P.FP8_TILES)
            continue
        split = C.c_int(-1)
        r = lib.eavqa_gemm_route(1 if c.dtype == "bf16" else 0, int(c.a_kc), int(c.b_kc), c.M, c.N, c.K, 0, c.knobs, C.byref(split))
        got = (r >> 8, r & 255, split.value) if r >= 0 else r
        if got != (c.kind, c.index, c.split):
            wrong[c.name] = (got, (c.kind, c.index, c.split))
        assert (c.kind, c.index) == P.TILES[c.tile][:2], c.name
    assert not wrong, wrong


def test_shapes_give_two_full_tiles_and_a_ragged_edge_each_way():
    for c in P.GEMM_CASES:
        if "nonlinear" in c.aspects or c.prefetch:
            continue
        bm, bn = P.FP8_TILES[c.fp8_tile - 1][:2] if c.dtype == "fp8" else P.TILES[c.tile][3:5]
        if c.kind == P.SKINNY:
            assert c.M <= 64 and c.N >= 2 * bn and c.N % bn, c.name
        else:
            assert c.M >= 2 * bm and c.M % bm and c.N >= 2 * bn and c.N % bn, c.name
        assert c.M * c.N <= 600 * 800 or c.split, c.name     # (the row split exists from 65 tile rows on)
        assert c.K <= 640, c.name


def test_tile_tables_are_the_kernels_own():
    """TILES / FP8_TILES (tile rows, columns, k per step, ring stages - what sizes the 'one more k-step than the ring has stages' cases)
    against the kernels' own tables and constants in csrc/: a kernel whose ring changes depth fails here until the probe follows."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "explicit-alignment-for-vqa-tasks_amd", "csrc")
    read = lambda f: open(os.path.join(csrc, f)).read()

    def table(src, name, launcher):
        body = src[re.search(r" " + name + r"\[\d*\] = \{", src).start():]
        body = body[:body.index("};")]
        rows = re.findall(r"\{(\d+), (\d+), [^{}]*?" + launcher + r"<([^>]*)>", body)
        return [(int(bm), int(bn), [t.strip() for t in targs.split(",")]) for bm, bn, targs in rows]

    k64 = table(read("gemm_k64.hip"), "K64_SHAPES", "launch_k64s")             # launch_k64s<WM, WN, MF, NF, NST, LW[, DB]>: 16 MF WM x 16 NF WN, BK = 64
    assert len(k64) == 11
    for i, (bm, bn, t) in enumerate(k64):
        wm, wn, mf, nf, nst = (int(x) for x in t[:5])
        assert (bm, bn) == (16 * mf * wm, 16 * nf * wn) and P.TILES[f"k64.{i}"][3:] == (bm, bn, 64, nst), i
    fp8 = table(read("gemm_fp8.hip"), "FP8_SHAPES", "launch_fp8")
    assert len(fp8) == len(P.FP8_TILES)
    for i, (bm, bn, t) in enumerate(fp8):
        wm, wn, mf, nf, nst = (int(x) for x in t[:5])
        assert (bm, bn) == (16 * mf * wm, 16 * nf * wn) and P.FP8_TILES[i] == (bm, bn, nst), i
    assert "const int nk = p.K >> 7;" in read("gemm_fp8.hip")                   # a stage row is 128 e4m3 values
    r1 = read("gemm_r1.hip")
    shaped = table(r1, "SHAPES", "launch_shaped")                              # launch_shaped<WM, WN, MF, NF>
    assert len(shaped) == 5
    for i, (bm, bn, t) in enumerate(shaped):
        wm, wn, mf, nf = (int(x) for x in t[:4])
        assert (bm, bn) == (16 * mf * wm, 16 * nf * wn) and P.TILES[f"shaped.{i}"][3:5] == (bm, bn), i
    # the round-1 kernels' rings are literals of their code, not table entries
    assert "constexpr int FBK = 32;" in r1 and "constexpr int GBM = 256, GBN = 256, GBK = 64;" in r1
    assert "gemm_bf16_fast_kernel<0, 4>" in r1 and P.TILES["fast"][3:] == (128, 128, 32, 4)
    assert "smem + (kt & 3) * G::STAGE" in r1 and all(P.TILES[f"shaped.{i}"][5:] == (32, 4) for i in range(5))
    assert "smem + (kt & 1) * GSTAGE" in r1 and P.TILES["big"][3:] == (256, 256, 64, 2)
    gen = read("gemm_general.hip")
    assert "constexpr int BM = 128, BN = 128;" in gen and "constexpr int BK16 = 64;" in gen and "constexpr int BK32 = 16;" in gen
    assert all(P.TILES[f"general.{i}"][3:6] == (128, 128, 64) and P.TILES[f"f32general.{i}"][3:6] == (128, 128, 16) for i in range(4))


# --------------------------------------------------------------------------------------------------------------------- coverage
def test_coverage_of_kinds_and_aspects():
    by_tile = {}
    for c in P.GEMM_CASES:
        by_tile.setdefault(c.tile, []).append(c)
    tiles = ["fast", "big", "skinny"] + [f"shaped.{i}" for i in range(5)] + [f"k64.{i}" for i in range(11)] + \
            [f"general.{i}" for i in range(4)] + [f"f32general.{i}" for i in range(4)] + [f"fp8.{i}" for i in range(5)]
    assert sorted(by_tile) == sorted(tiles)
    for t in tiles:
        cs = by_tile[t]
        n = Counter(a for c in cs for a in c.aspects)
        flags = Counter()
        for c in cs:
            f = c.vec_flags()
            if f.count(False) == 1 and c.aux and c.res and c.bias is not None:
                flags[("vec_c", "vec_aux", "vec_res", "vec_bias")[f.index(False)]] += 1        # this flag 0 on its own
            if f.count(False) == 4:
                flags["all"] += 1
        assert n["strided"] >= 2 and n["guards"] >= 1 and n["head"] >= 2, (t, n)
        assert all(flags[k] >= 1 for k in ("vec_c", "vec_aux", "vec_res", "vec_bias", "all")), (t, flags)
        bk, stages = (128, P.FP8_TILES[int(t[4:])][2]) if t.startswith("fp8") else P.TILES[t][5:7]
        assert any("strided" in c.aspects and c.K == bk for c in cs), t                    # one k-step
        if t != "skinny":
            assert any("strided" in c.aspects and c.K == bk * (stages + 1) for c in cs), t     # one more than the ring has stages
        if not t.startswith("fp8"):
            outs = {c.out for c in cs if "inplace" in c.aspects and c.res == "inplace" and not c.vec_flags()[0] and c.ldc > c.N}
            assert "f32" in outs and (t.startswith("f32") or outs & {"bf16", "f16"}), (t, outs)     # float32 and 16-bit, strided and unaligned
        assert any(c.aux == "in" for c in cs) and any(c.aux == "out" for c in cs), t
        assert any("head" in c.aspects and c.alpha != 1.0 and c.ldc > c.N and c.ldc % 4 == 0 and (c.N % 2 == 1 or not c.b_kc) for c in cs), t
        if not (t.startswith("f32") or t.startswith("fp8")):
            assert {c.out for c in cs} == {"f32", "bf16", "f16"} and {c.res_dtype for c in cs if c.res} == {"f32", "bf16", "f16"}, t
    assert sum(c.split > 0 for c in P.GEMM_CASES) >= 1 and sum(c.prefetch for c in P.GEMM_CASES) == 1
    assert any(c.kind == P.BIG and c.knobs & P.NO_ROW_SPLIT for c in P.GEMM_CASES)
    assert any(c.kind in (P.GEN, P.F32) and c.N in (784, 785) and c.K % 64 for c in P.GEMM_CASES)
    nl = Counter((c.tile, c.act) for c in P.GEMM_CASES if "nonlinear" in c.aspects)
    assert len(nl) == 6 * 3 and set(nl.values()) == {3}
    # the decode step's kernels
    sk = [c for c in P.SPLITK_CASES if not c.fp8]
    forced = {P.splitk_variant(c.sel) for c in sk if c.sel}                 # decoded (U, NW, NF): two selector words may name one kernel
    assert forced == {(U, NW, NF) for U in (8, 16) for NW in (4, 8) for NF in (1, 2)} and len(P.SPLITK_SELS) == 8 and any(c.sel == 0 for c in sk)
    assert {c.ks for c in sk} == {0, 1, 2, 3} and {c.M for c in sk} >= set(P.SPLITK_MS)
    for U, NW, NF in forced:
        mine = [c for c in sk if c.sel and P.splitk_variant(c.sel) == (U, NW, NF)]
        assert {c.nsteps for c in mine} == {1, U - 1, U, U + 1, 2 * U + 1}
        assert all(c.N % (16 * NW * NF) and c.N > 16 * NW * NF and c.U == U for c in mine)          # ragged against the workgroup's columns
    assert {c.U for c in P.SPLITK_CASES if c.fp8} == {4, 8} and any(c.fp8 and c.ks == 0 for c in P.SPLITK_CASES)
    fin = [c for c in P.FINISH_CASES if not c.gated]
    assert {(c.n_seg, c.ks, c.out) for c in fin} == {(s, k, o) for s in (1, 2, 3) for k in P.FINISH_KS for o in ("f32", "bf16")}
    assert {c.act for c in fin} == set(P.ACTS) and any(c.ldr > c.N for c in fin) and any(c.ldr == 0 for c in fin)
    gated = [c for c in P.FINISH_CASES if c.gated]
    assert {(c.ks, c.out) for c in gated} == {(k, o) for k in P.FINISH_KS for o in ("f32", "bf16")} and {c.act for c in gated} == set(P.ACTS)
    dd = P.DECODE_CASES
    assert {c.sel & 0xF for c in dd if not c.gated} == {1, 2, 3, 4} and any(c.sel & 0x80 for c in dd)
    assert sum(c.gated and c.bias for c in dd) >= 4 and any(c.n_seg == 3 and (c.N // 3) % 16 for c in dd)
    assert any(c.want_stats and c.N % (16 * (c.sel & 0xF)) for c in dd)


# -------------------------------------------------------------------------------------------------------------------- mutations
def _first(pred):
    return next(c for c in P.GEMM_CASES if c.a_kc and c.b_kc and c.act in P.EXACT_ACTS and c.M <= 600 and pred(c))


GEMM_MUTATION_CASES = {
    "lda_is_K": lambda c: "strided" in c.aspects,
    "chunk_past_K": lambda c: "strided" in c.aspects,
    "store4_at_ragged_N": lambda c: "head" in c.aspects and c.N % 4 and c.out == "f32",
    "row_M_written": lambda c: "guards" in c.aspects,
    "residual_ldc": lambda c: "guards" in c.aspects and c.res == "f32",
    "aux_out_ldc": lambda c: "guards" in c.aspects and c.aux == "out",
    "bias_rounded_down": lambda c: c.bias == 1,
}


@pytest.mark.parametrize("mutation", P.GEMM_MUTATIONS)
@pytest.mark.parametrize("dtype", ["bf16", "f32", "fp8"])
def test_gemm_mutations_are_rejected(mutation, dtype):
    pick = GEMM_MUTATION_CASES[mutation]
    c = _first(lambda c: c.dtype == dtype and pick(c))
    bufs, v = P.materialize(c)
    ref = P.reference(c, bufs, v)
    good = copy.deepcopy(bufs)
    P.emulate_gemm(c, good)
    P.check(c, ref, good)                                   # the emulation itself passes ...
    bad = copy.deepcopy(bufs)
    P.emulate_gemm(c, bad, mutation)
    with pytest.raises(AssertionError):                     # ... and its mutation does not
        P.check(c, ref, bad)


def test_emulation_passes_every_exact_gemm_case_of_two_kernels(gemm_refs):
    """The unmutated emulation agrees with the reference on every aspect (strides, offsets, in place, every output type)."""
    n = 0
    for c in P.GEMM_CASES:
        if c.tile in ("k64.0", "f32general.0", "fp8.0", "skinny") and c.act in P.EXACT_ACTS:
            bufs, v, ref = gemm_refs[c.name]
            got = copy.deepcopy(bufs)
            P.emulate_gemm(c, got)
            P.check(c, ref, got)
            n += 1
    assert n >= 30


@pytest.mark.parametrize("mutation", P.SPLITK_MUTATIONS)
@pytest.mark.parametrize("fp8", [False, True])
def test_splitk_mutations_are_rejected(lib, mutation, fp8):
    c = next(c for c in P.SPLITK_CASES if c.fp8 == fp8 and c.ks >= 2 and c.nsteps % c.U and c.nsteps > 1)
    ks, KS = c.resolve()
    bufs, v = P.materialize_splitk(c, ks, KS)
    ref = P.reference_splitk(c, ks, KS, bufs, v)
    good, bad = copy.deepcopy(bufs), copy.deepcopy(bufs)
    P.emulate_splitk(c, ks, KS, good)
    P.check_splitk(c, ks, ref, good)
    P.emulate_splitk(c, ks, KS, bad, mutation)
    with pytest.raises(AssertionError):
        P.check_splitk(c, ks, ref, bad)


@pytest.mark.parametrize("mutation", P.FINISH_MUTATIONS)
@pytest.mark.parametrize("out", ["f32", "bf16"])
def test_finish_mutations_are_rejected(mutation, out):
    want = (lambda c: c.ks == 9) if mutation == "first_8_slices" else (lambda c: c.n_seg >= 2)
    c = next(c for c in P.FINISH_CASES if c.out == out and c.act in P.EXACT_ACTS and want(c))
    bufs, v = P.materialize_finish(c)
    ref = P.reference_finish(c, v)
    good, bad = copy.deepcopy(bufs), copy.deepcopy(bufs)
    P.emulate_finish(c, good)
    P.check_finish(c, ref, good)
    P.emulate_finish(c, bad, mutation)
    with pytest.raises(AssertionError):
        P.check_finish(c, ref, bad)


@pytest.mark.parametrize("mutation", P.DECODE_MUTATIONS)
def test_decode_mutations_are_rejected(mutation):
    for c in (c for c in P.DECODE_CASES if c.gated and c.bias):
        bufs, v = P.materialize_decode(c)
        ref = P.reference_decode(c, v)
        good, bad = copy.deepcopy(bufs), copy.deepcopy(bufs)
        P.emulate_decode(c, good)
        P.check_decode(c, ref, good)
        P.emulate_decode(c, bad, mutation)
        with pytest.raises(AssertionError):
            P.check_decode(c, ref, bad)


def test_twelve_mutations():
    assert len(P.GEMM_MUTATIONS) + len(P.SPLITK_MUTATIONS) + len(P.FINISH_MUTATIONS) + len(P.DECODE_MUTATIONS) == 12


def test_ln_splitk_table():
    assert max(P.LN_COLS) == 16384 and P.LN_COLS_REJECTED == 16388
    nv = {(c // 4 + 511) // 512 for c in P.LN_COLS}         # float4 per thread, rounded up to the instantiated 1, 2, 4, 8 by the launcher
    assert {1, 2} <= nv and any(2 < n <= 4 for n in nv) and any(4 < n <= 8 for n in nv)
    assert (P.LN_COLS_REJECTED // 4 + 511) // 512 > 8 and {0, 1, 7, 8, 9, 16, 17} == set(P.LN_KS)
