"""GPU: the sequence-assembly kernels (csrc/seq.hip) on the exact probes of tests/_seq_probe.py.

Every entry point is called through `_lib.call` with the pointers and strides of windows into flat buffers: input pads hold NaN (or a
poison id), output pads and a guard row a sentinel.  The expectation is equality with a plain reference - positions, mask bits and
status of every row layout around the 64-token chunk edges, labels around the carry of their two scans, every 1024-column pass of
the embedding gathers and their backward, strided row moves, both transpose kernels with ragged tiles and their fallbacks, T5's gate
beyond its first grid-stride pass - and that nothing outside the output windows was written.  The real-valued legs of the gate are
bounded per element by the tolerance of test_gated_activation_forward_backward.  Where an `ops` wrapper exists, it runs once on the
same data held contiguously and must return the same bits.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _seq_probe as S

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as _ops, _lib
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    return _ops


def to_dev(bufs):
    return {nm: S.on_device(b, vw, DEV) for nm, (b, vw) in bufs.win.items()}


def back(bufs, dev, names):
    got = S.Bufs()
    for nm in names:
        vw = bufs.win[nm][1]
        b = dev[nm][0].cpu()
        got.win[nm] = (b, b.as_strided(tuple(vw.shape), vw.stride(), vw.storage_offset()))
    return got


def collect(cases, run):
    assert cases
    failed = []
    for c in cases:
        try:
            run(c)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def pointers(dev):
    return lambda nm: dev[nm][1].data_ptr() if nm in dev else None


def same_bits(name, what, window_view, wrapped):
    a, b = window_view.contiguous(), wrapped.cpu().reshape(window_view.shape)
    as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    assert a.dtype == b.dtype and torch.equal(a.view(as_int), b.view(as_int)), f"{name}: ops.{what} returns other bits than the strided call"


# --------------------------------------------------------------------------------------------------------------- row builders
def run_rows(ops, c):
    from eavqa_amd import _lib
    bufs, v = S.materialize_rows(c)
    ref = S.reference_rows(c, v)
    dev = to_dev(bufs)
    p = pointers(dev)
    if c.kind == "fewshot":
        _lib.call("eavqa_build_fewshot_rows", c.B, c.T, c.L, c.n_img, S.SPECIAL, p("tokens"), p("qmask"), c.pos_mode, p("src"), p("mask"), p("pos"),
                  p("status"), ops._stream())
    else:
        _lib.call("eavqa_build_prefix_rows", c.B, c.L, c.T, p("tokens"), p("qmask"), c.pos_mode, c.stride, c.offset, p("src"), p("mask"), p("pos"),
                  ops._stream())
    names = S.ROW_OUTPUTS[c.kind]
    got = back(bufs, dev, names)
    S.check_rows(c, ref, got)
    if c.T == 0:
        return
    tok, qm = torch.from_numpy(v["tokens"]).to(DEV), torch.from_numpy(v["qmask"]).to(DEV)
    if c.kind == "fewshot":
        outs = ops.build_fewshot_rows(tok, qm, c.L, c.n_img, S.SPECIAL, c.pos_mode)
    else:
        outs = ops.build_prefix_rows(tok, qm, c.L, c.pos_mode, c.stride, c.offset)
    for nm, o in zip(names, outs):
        same_bits(c.name, f"build_{c.kind}_rows ({nm})", got.win[nm][1], o)


@pytest.mark.parametrize("T", S.FEWSHOT_T)
def test_fewshot_rows(ops, T):
    collect([c for c in S.FEWSHOT_CASES if c.T == T], lambda c: run_rows(ops, c))


def test_prefix_rows(ops):
    collect(S.PREFIX_CASES, lambda c: run_rows(ops, c))


# --------------------------------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("T", S.LABELS_T)
def test_labels(ops, T):
    from eavqa_amd import _lib

    def run(c):
        bufs, v = S.materialize_labels(c)
        ref = S.ref_labels(v["ids"], c.L, S.PAD, c.bos, c.mode)
        dev = to_dev(bufs)
        p = pointers(dev)
        _lib.call("eavqa_build_labels", c.mode, v["ids"].shape[0], c.T, c.L, p("ids"), S.PAD, c.bos, p("out"), ops._stream())
        got = back(bufs, dev, ["out"])
        S.check_labels(c, ref, got)
        same_bits(c.name, "build_labels", got.win["out"][1], ops.build_labels(torch.from_numpy(v["ids"]).to(DEV), c.L, S.PAD, c.bos, c.mode))
    collect([c for c in S.LABELS_CASES if c.T == T], run)


# ---------------------------------------------------------------------------------------------------------------------- embed
@pytest.mark.parametrize("E", S.EMBED_E)
def test_embed_assemble_and_backward(ops, E):
    from eavqa_amd import _lib

    def run(c):
        bufs, v = S.materialize_embed(c)
        ref = S.reference_embed(c, v)
        dev = to_dev(bufs)
        p = pointers(dev)
        rows, dt = len(v["src"]), ops.dtype_id(S.DT[c.dtype])
        _lib.call("eavqa_embed_assemble", dt, rows, c.E, p("src"), p("pos"), p("wte"), c.ld("wte"), p("prefix"), c.ld("prefix"), p("wpe"),
                  c.ld("wpe") if c.wpe else 0, p("x"), c.ld("x"), ops._stream())
        _lib.call("eavqa_embed_assemble_bwd", dt, rows, c.E, p("src"), p("dx"), c.ld("dx"), p("dprefix"), c.ld("dprefix"), ops._stream())
        got = back(bufs, dev, ["x", "dprefix"])
        S.check_embed(c, ref, got)
        src, pos = dev["src"][1][0], dev["pos"][1][0]
        x = ops.embed_assemble(src, pos, dev["wte"][1].contiguous(), dev["prefix"][1].contiguous(), dev["wpe"][1].contiguous() if c.wpe else None)
        same_bits(c.name, "embed_assemble", got.win["x"][1], x)
        d = ops.embed_assemble_bwd(src, dev["dx"][1].contiguous(), ref["named"].numel(), S.DT[c.dtype])
        same_bits(c.name, "embed_assemble_bwd (named rows)", got.win["dprefix"][1][ref["named"]], d[ref["named"].to(DEV)])
        assert not d[(~ref["named"]).to(DEV)].any(), f"{c.name}: ops.embed_assemble_bwd wrote a prefix row that src does not name"
    collect([c for c in S.EMBED_CASES if c.E == E], run)


# ----------------------------------------------------------------------------------------------------------------------- move
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_move_rows(ops, dtype):
    from eavqa_amd import _lib

    def run(c):
        bufs, v = S.materialize_move(c)
        ref = S.reference_move(c, v)
        dev = to_dev(bufs)
        p = pointers(dev)
        _lib.call("eavqa_move_rows", ops.dtype_id(S.DT[c.dtype]), int(c.scatter), c.n, c.cols, p("src"), c.ld_src, p("idx"), p("dst"), c.ld_dst, ops._stream())
        got = back(bufs, dev, ["dst"])
        S.check_move(c, ref, got)
        src, idx = dev["src"][1].contiguous(), dev["idx"][1][0]
        if c.scatter:
            out = ops.scatter_rows(src, idx, v["dst_rows"])
            assert not out[(~ref[1]).to(DEV)].any(), f"{c.name}: ops.scatter_rows wrote a row that idx does not name"
            same_bits(c.name, "scatter_rows", got.win["dst"][1][ref[1]], out[ref[1].to(DEV)])
        else:
            same_bits(c.name, "gather_rows", got.win["dst"][1], ops.gather_rows(src, idx))
    collect([c for c in S.MOVE_CASES if c.dtype == dtype], run)


def test_move_rows_empty_and_misaligned(ops):
    """n = 0: OK, nothing written.  A pointer off 16 bytes, a row stride or a width that is no whole number of 16-byte vectors:
    EAVQA_E_ALIGN, nothing written."""
    from eavqa_amd import _lib
    lib = _lib.load()
    for dtype, cols, ld_src, ld_dst, src_off, dst_off in S.MOVE_REJECTED + (("bf16", 8, 16, 24, 0, 0), ("f32", 4, 8, 12, 0, 0)):
        accepted = S.move_accepts(dtype, cols, ld_src, ld_dst, src_off, dst_off)
        for scatter in (0, 1):
            sb, sv = S.on_device(*S.window(3, cols, ld_src, S.DT[dtype], elem_offset=src_off, fill=1.0), DEV)
            db, dv = S.on_device(*S.window(3, cols, ld_dst, S.DT[dtype], elem_offset=dst_off, fill=S.SENTINEL), DEV)
            idx = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
            rc = lib.eavqa_move_rows(ops.dtype_id(S.DT[dtype]), scatter, 0 if accepted else 3, cols, sv.data_ptr(), ld_src, idx.data_ptr(), dv.data_ptr(),
                                     ld_dst, ops._stream())
            torch.cuda.synchronize()
            tag = (dtype, cols, ld_src, ld_dst, src_off, dst_off, scatter)
            assert rc == (0 if accepted else _lib.EAVQA_E_ALIGN), tag
            d = db.cpu()
            assert bool((d == S.SENTINEL).all()), tag


# ------------------------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_transpose(ops, dtype):
    from eavqa_amd import _lib

    def run(c):
        bufs, v = S.materialize_transpose(c)
        ref = S.ref_transpose(v["x"])
        dev = to_dev(bufs)
        p = pointers(dev)
        assert dev["src"][0].data_ptr() % 16 == 0 and dev["dst"][0].data_ptr() % 16 == 0        # (`c.fast` assumes aligned backing buffers)
        _lib.call("eavqa_transpose", ops.dtype_id(S.DT[c.dtype]), c.rows, c.cols, p("src"), c.ld_src, p("dst"), c.ld_dst, ops._stream())
        got = back(bufs, dev, ["dst"])
        S.check_transpose(c, ref, got)
        if c.src_off == c.dst_off == 0:
            same_bits(c.name, "transpose", got.win["dst"][1], ops.transpose(dev["src"][1].contiguous()))
    collect([c for c in S.TRANSPOSE_CASES if c.dtype == dtype], run)


# ---------------------------------------------------------------------------------------------------------------------- gated
@pytest.mark.parametrize("rows", [s[0] for s in S.GATED_SHAPES])
def test_gated_activation(ops, rows):
    from eavqa_amd import _lib

    def run(c):
        bufs, v = S.materialize_gated(c)
        ref = S.reference_gated(c, v)
        dev = to_dev(bufs)
        p = pointers(dev)
        dt, act = ops.dtype_id(S.DT[c.dtype]), _lib.ACT[c.act]
        _lib.call("eavqa_gated_act_fwd", dt, c.rows, c.F, act, p("u"), c.ldu, p("h"), c.ldh, ops._stream())
        _lib.call("eavqa_gated_act_bwd", dt, c.rows, c.F, act, p("u"), c.ldu, p("dh"), c.lddh, p("du"), c.lddu, ops._stream())
        got = back(bufs, dev, ["h", "du"])
        S.check_gated(c, ref, got)
        u = dev["u"][1].contiguous()
        same_bits(c.name, "gated_act_fwd", got.win["h"][1], ops.gated_act_fwd(u, c.act))
        same_bits(c.name, "gated_act_bwd", got.win["du"][1], ops.gated_act_bwd(u, dev["dh"][1].contiguous(), c.act))
    collect([c for c in S.GATED_CASES if c.rows == rows], run)
    print("worst error / bound of the real-valued legs so far:", {k: round(x, 4) for k, x in sorted(S.WORST.items())})


# ------------------------------------------------------------------------------------------------------------------------ vit
@pytest.mark.parametrize("kind", ["patchify", "assemble"])
def test_vit_inputs(ops, kind):
    from eavqa_amd import _lib

    def run(c):
        bufs, v = S.materialize_vit(c)
        ref = S.reference_vit(c, v)
        dev = to_dev(bufs)
        p = pointers(dev)
        dt = ops.dtype_id(S.DT[c.dtype])
        if c.kind == "patchify":
            _lib.call("eavqa_patchify", dt, c.B, c.img, c.ps, p("px"), p("out"), c.ldp, ops._stream())
            got = back(bufs, dev, ["out"])
            S.check_vit(c, ref, got)
            same_bits(c.name, "patchify", got.win["out"][1], ops.patchify(v["px"].float().to(DEV), c.ps, S.DT[c.dtype], c.ldp))
        else:
            _lib.call("eavqa_vit_assemble", dt, c.B, c.n_patch, c.W, p("pe"), c.ldpe, p("cls"), p("pos"), p("x"), c.ldx, ops._stream())
            got = back(bufs, dev, ["x"])
            S.check_vit(c, ref, got)
            x = ops.vit_assemble(dev["pe"][1].contiguous(), v["cls"][0].float().to(DEV), v["pos"].float().to(DEV), c.B, c.n_patch)
            same_bits(c.name, "vit_assemble", got.win["x"][1], x)
    collect([c for c in S.VIT_CASES if c.kind == kind], run)
