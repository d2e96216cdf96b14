"""Exact probes of the sequence-assembly kernels (csrc/seq.hip): the row builders, the label masks, the embedding gathers, the row moves,
the transposes, T5's gate and the ViT input assembly - case tables, plain references, acceptance functions (no GPU needed here).

Conventions of tests/_gemm_probe.py: every matrix of a call is a window into a flat buffer.  Input pads hold NaN - for the integer
inputs of the row builders a poison id, which no vocabulary holds and which reads as "attended" in a mask - and output pads plus one
guard row hold SENTINEL (int32 / int64 outputs: an int poison); `untouched` tells whether a kernel wrote one of them.  Float operands
are small integers (|v| <= 8 in bf16, <= 256 in float32): every copy, cast, product and two-term sum of a case is exact, and the
expectation is equality with the reference.  The references are loops over rows and columns in float64 / Python integers; they share
no code with the emulations further down, which walk the data as the kernels do (64-wide chunks with a carry, 1024-column passes,
grid-stride passes, 64 x 64 tiles) and take one-line mutations that tests/test_seq_probe_cpu.py requires the acceptance functions
to reject.
"""
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import oracle
from _gemm_probe import ACT_F, EXACT_ACTS, NAN, NONLINEAR, SENTINEL, Bufs, _first_diff, act_grad, on_device, untouched, window  # noqa: F401

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LIM = {"f32": 256, "bf16": 8}                # |v| of the integer data
POISON_ID = 0x5A5A5A5A5A                     # pads of int64 inputs: outside every vocabulary (as int32: 0x5A5A5A5A), non-zero as a mask bit
POISON_I32 = -0x5A5A5A5                      # pads and guard rows of int32 outputs: no source row, no mask bit, no position, no count
POISON_I64 = -0x5A5A5A5A5A5                  # the same of int64 outputs (labels)
SPECIAL = 40                                 # the first sentinel id of the few-shot cases; the window is SPECIAL - i, i < n_img <= 5
VOCAB = 44                                   # rows of the token table the embed cases gather from: SPECIAL + 1 is an ordinary token
TEXT_HI = 34                                 # random text ids are 1 .. TEXT_HI: below SPECIAL - 5, the lowest sentinel id of any case


def _rng(name: str) -> np.random.RandomState:
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def pattern(rows: int, cols: int, lim: int, a: int, b: int, shift: int = 0):
    """float64 integers in [-lim, lim], a function of (row, column) with different steps along the two axes: a swapped, shifted or
    repeated row or column changes it."""
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    return ((a * r + b * c + shift) % (2 * lim + 1) - lim).double()


def _first(got, want):
    """'first difference at (row, column)' of two equal-shaped integer / float arrays."""
    got, want = np.asarray(got), np.asarray(want)
    bad = got != want
    if got.dtype.kind == "f":
        bad |= np.isnan(got)
    if not bad.any():
        return "none"
    i = tuple(int(x) for x in np.argwhere(bad)[0])
    return f"{int(bad.sum())} elements differ, first at {i}: got {got[i]}, want {want[i]}"


def _view_np(win):
    bk, vw = win
    return (vw.double() if vw.is_floating_point() else vw.long()).numpy()


def _geo(bufs, nm):
    vw = bufs.win[nm][1]
    return vw.storage_offset(), vw.stride(0)


def _in(bufs, nm):
    """The whole flat input buffer as float64 / int64, pads included."""
    b = bufs.win[nm][0]
    return (b.double() if b.is_floating_point() else b.long()).numpy()


def _rd(flat, idx):
    return np.take(flat, idx, mode="clip")


def _i32(v: int) -> int:
    """(int)v of a 64-bit value."""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


class _Out:
    """A flat output buffer an emulation writes by element index.  An index outside the buffer lands on its first / last element, which is
    a guard, so `untouched` sees it."""

    def __init__(self, bufs, nm):
        self.b = bufs.win[nm][0]
        self.off, self.ld = _geo(bufs, nm)
        self.lowp = self.b.dtype == torch.bfloat16
        self.a = self.b.float().numpy() if self.lowp else self.b.numpy()          # (SENTINEL and the integers survive the round trip)

    def put(self, idx, vals):
        self.a[np.clip(np.asarray(idx), 0, self.a.size - 1)] = vals

    def flush(self):
        if self.lowp:
            self.b.copy_(torch.from_numpy(self.a))


# ============================================================================================================== row builders
def positions(mask_row, pos_mode: int):
    """GPT-2: arange; OPT: cumsum(mask) * mask - 1 + 2."""
    out, run = [], 0
    for s, m in enumerate(mask_row):
        run += int(m)
        out.append(s if pos_mode == 0 else run * int(m) - 1 + 2)
    return out


def ref_prefix_rows(tokens, qmask, L: int, pos_mode: int, stride: int, offset: int):
    """-> (src, mask, pos) int64 [B, L + T]: row b is the L prefix vectors -(1 + b * stride + offset + l) followed by its tokens."""
    B = len(qmask)
    T = len(qmask[0]) if B else 0
    src, mask, pos = [], [], []
    for b in range(B):
        s_row = [-(1 + b * stride + offset + l) for l in range(L)] + [int(tokens[b][t]) for t in range(T)]
        m_row = [1] * L + [1 if int(qmask[b][t]) != 0 else 0 for t in range(T)]
        src.append(s_row)
        mask.append(m_row)
        pos.append(positions(m_row, pos_mode))
    shape = (B, L + T)
    return tuple(np.asarray(x, dtype=np.int64).reshape(shape) for x in (src, mask, pos))


def ref_fewshot_rows(tokens, qmask, L: int, n_img: int, special: int, pos_mode: int):
    """-> (src, mask, pos [B, T + (L - 1) n_img], status [B]): the walk of oracle.insert_prefix_into_input over every row, with what the
    kernel documents for rows the oracle refuses: sentinel number n_img + 1 and later leave their L slots unwritten (0, mask 0) and
    still count in status; the tail of a row with too few sentinels is 0 / mask 0; text that would land at or past T_out is dropped."""
    B, T = len(tokens), len(tokens[0])
    T_out = T + (L - 1) * n_img
    sentinels = {special - i for i in range(n_img)}
    src = np.zeros((B, T_out), dtype=np.int64)
    mask = np.zeros((B, T_out), dtype=np.int64)
    pos = np.zeros((B, T_out), dtype=np.int64)
    status = np.zeros(B, dtype=np.int64)
    for b in range(B):
        o = n = 0
        for t in range(T):
            if int(tokens[b][t]) in sentinels:
                if n < n_img:
                    for l in range(L):
                        src[b, o + l] = -(1 + (b * n_img + n) * L + l)
                        mask[b, o + l] = 1
                o += L
                n += 1
            else:
                if o < T_out:
                    src[b, o] = int(tokens[b][t])
                    mask[b, o] = 1 if int(qmask[b][t]) != 0 else 0
                o += 1
        status[b] = n
        pos[b] = positions(mask[b], pos_mode)
    return src, mask, pos, status


def mask_row(shape: str, T: int):
    m = np.ones(T, dtype=np.int64)
    if shape == "right":
        m[T - max(1, T // 4):] = 0
    elif shape == "left":
        m[:max(1, T // 4)] = 0
    elif shape == "holes":
        m[[t for t in range(T) if t % 5 == 2 or t in (62, 65)]] = 0
    elif shape != "ones":
        raise ValueError(shape)
    return m


# (name, preferred sentinel columns (-1: T - 1), count as a function of n_img, mask shape, ids in reverse order)
FEWSHOT_ROWS = (
    ("edges", (0, -1, 63, 64), lambda n: n, "right", False),
    ("straddle", (63, 64, 0), lambda n: n, "left", False),
    ("chunk-start", (64, 0, -1), lambda n: n, "holes", False),
    ("near-ids", (63, -1), lambda n: n, "ones", False),                 # + SPECIAL + 1 and SPECIAL - n_img as text
    ("masked-sentinel", (-1, 0, 64, 63), lambda n: n, "ones", True),    # + mask bit 0 on every sentinel
    ("too-few", (64, 0), lambda n: n - 1, "right", False),
    ("scattered", (65, 62), lambda n: n, "left", True),
    ("too-many", (0, 63, 64, 65), lambda n: 2 * n, "holes", False),     # the last row: what it writes past its end lands in the guard row
)


@dataclass(frozen=True)
class RowsCase:
    name: str
    kind: str                       # fewshot | prefix
    B: int
    T: int
    L: int
    pos_mode: int
    n_img: int = 0                  # fewshot
    stride: int = 0                 # prefix
    offset: int = 0

    @property
    def S(self):
        return self.T + (self.L - 1) * self.n_img if self.kind == "fewshot" else self.L + self.T


def _place(T: int, n: int, preferred, rng):
    cols = []
    for p in preferred:
        p = T - 1 if p < 0 else p
        if 0 <= p < T and p not in cols and len(cols) < n:
            cols.append(p)
    rest = [c for c in rng.permutation(T).tolist() if c not in cols]
    return sorted(cols + rest[:max(0, n - len(cols))])


def row_inputs(c: RowsCase):
    """(tokens, qmask int64 [B, T], facts): `facts[b]` names what row b's layout exercises (the coverage assertions read it)."""
    rng = _rng(c.name)
    tokens = rng.randint(1, TEXT_HI + 1, size=(c.B, c.T)).astype(np.int64)
    qmask = np.ones((c.B, c.T), dtype=np.int64)
    facts = []
    if c.kind == "prefix":
        for b, shape in enumerate(("right", "left", "holes", "ones")[:c.B]):
            if c.T:
                qmask[b] = mask_row(shape, c.T)
            facts.append({f"mask:{shape}"})
        return tokens, qmask, facts
    for b, (name, pref, count, shape, rev) in enumerate(FEWSHOT_ROWS):
        sc = _place(c.T, count(c.n_img), pref, rng)
        for i, t in enumerate(sc):
            k = i % c.n_img
            tokens[b, t] = SPECIAL - (c.n_img - 1 - k if rev else k)
        qmask[b] = mask_row(shape, c.T)
        f = {name, f"mask:{shape}"}
        free = [t for t in range(c.T) if t not in sc]
        if name == "near-ids" and len(free) >= 2:
            tokens[b, free[len(free) // 2]] = SPECIAL + 1
            tokens[b, free[len(free) // 3]] = SPECIAL - c.n_img
            f.add("near-ids-as-text")
        if name == "masked-sentinel":
            qmask[b, sc] = 0
        f |= {f"sent@{t}" for t in sc if t in (0, 63, 64)}
        if c.T - 1 in sc:
            f.add("sent@T-1")
        if 63 in sc and 64 in sc:
            f.add("sent@63|64")
        if any(qmask[b, t] == 0 for t in sc):
            f.add("mask-0-on-sentinel")
        if len(sc) < c.n_img:
            f.add("under-full")
        if len(sc) > c.n_img:
            f.add("over-full")
        if len(sc) == 2 * c.n_img:
            f.add("twice-n_img")
        if len({int(tokens[b, t]) for t in sc}) == c.n_img and len(sc) >= c.n_img:
            f.add("every-id-of-the-window")
        facts.append(f)
    return tokens, qmask, facts


def well_formed(c: RowsCase, tokens):
    """Rows the oracle accepts: exactly n_img sentinels."""
    return [b for b in range(c.B) if int(((tokens[b] <= SPECIAL) & (tokens[b] > SPECIAL - c.n_img)).sum()) == c.n_img]


FEWSHOT_T, FEWSHOT_L, FEWSHOT_NIMG = (1, 63, 64, 65, 130), (1, 2, 10), (1, 3, 5)
FEWSHOT_CASES = [RowsCase(f"fewshot-T{T}-L{L}-n{n}-pos{pm}", "fewshot", len(FEWSHOT_ROWS), T, L, pm, n_img=n)
                 for T in FEWSHOT_T for L in FEWSHOT_L for n in FEWSHOT_NIMG for pm in (0, 1)]
PREFIX_LT = ((0, 5), (10, 0), (1, 63), (10, 54), (10, 55), (70, 70))
PREFIX_CASES = []
for _L, _T in PREFIX_LT:
    for _st, _of in sorted({(_L, 0), (3 * _L, _L), (3 * _L, 2 * _L)}):
        for _pm in (0, 1):
            PREFIX_CASES.append(RowsCase(f"prefix-L{_L}-T{_T}-stride{_st}-off{_of}-pos{_pm}", "prefix", 4, _T, _L, _pm, stride=_st, offset=_of))
ROW_OUTPUTS = {"fewshot": ("src", "mask", "pos", "status"), "prefix": ("src", "mask", "pos")}


def materialize_rows(c: RowsCase):
    tokens, qmask, _ = row_inputs(c)
    bufs = Bufs()
    if c.T > 0:
        for nm, x, off in (("tokens", tokens, 3), ("qmask", qmask, 1)):
            bk, vw = window(c.B, c.T, c.T, torch.int64, elem_offset=off, fill=POISON_ID)
            vw.copy_(torch.from_numpy(x))
            bufs.win[nm] = (bk, vw)
    for nm, off in (("src", 1), ("mask", 2), ("pos", 3)):
        bufs.win[nm] = window(c.B, c.S, c.S, torch.int32, elem_offset=off, fill=POISON_I32)
    if c.kind == "fewshot":
        bufs.win["status"] = window(1, c.B, c.B, torch.int32, elem_offset=1, fill=POISON_I32)
    return bufs, {"tokens": tokens, "qmask": qmask}


def reference_rows(c: RowsCase, v):
    if c.kind == "fewshot":
        return dict(zip(ROW_OUTPUTS["fewshot"], ref_fewshot_rows(v["tokens"], v["qmask"], c.L, c.n_img, SPECIAL, c.pos_mode)))
    return dict(zip(ROW_OUTPUTS["prefix"], ref_prefix_rows(v["tokens"], v["qmask"], c.L, c.pos_mode, c.stride, c.offset)))


def check_rows(c: RowsCase, ref, got: Bufs):
    for nm in ROW_OUTPUTS[c.kind]:
        bk, vw = got.win[nm]
        assert untouched(bk, vw, POISON_I32), f"{c.name}: {nm} was written outside its rows"
        g = _view_np(got.win[nm]).reshape(ref[nm].shape)
        assert np.array_equal(g, ref[nm]), f"{c.name}: {nm}: {_first(g, ref[nm])}"


ROW_MUTATIONS = ("pos_carry_dropped", "pos_without_mask_multiply", "sentinel_carry_dropped", "before_inclusive", "slot_mask_from_question_mask",
                 "overfull_row_writes_its_extra_sentinel", "text_written_past_T_out", "status_capped_at_n_img", "stride_ignored", "offset_ignored")


def _iscan64(v):
    out, run = [], 0
    for x in v:
        run += x
        out.append(run)
    return out


def _emulate_positions(lds, S, pos_mode, pos: _Out, base, mutation):
    carry = 0
    for s0 in range(0, S, 64):
        mv = [lds[s0 + lane] if s0 + lane < S else 0 for lane in range(64)]
        inc = [x + (0 if mutation == "pos_carry_dropped" else carry) for x in _iscan64(mv)]
        for lane in range(64):
            s = s0 + lane
            if s < S:
                opt = inc[lane] - 1 + 2 if mutation == "pos_without_mask_multiply" else inc[lane] * mv[lane] - 1 + 2
                pos.put(base + s, s if pos_mode == 0 else opt)
        carry = inc[63]


def emulate_rows(c: RowsCase, bufs: Bufs, mutation: Optional[str] = None):
    """prefix_rows_kernel / fewshot_rows_kernel: one 64-lane wave per row, the mask row in LDS, chunks of 64 with a carry."""
    T, L, S = c.T, c.L, c.S
    tok = _in(bufs, "tokens") if T else None
    qm = _in(bufs, "qmask") if T else None
    t_off = _geo(bufs, "tokens")[0] if T else 0
    q_off = _geo(bufs, "qmask")[0] if T else 0
    src, msk, pos = _Out(bufs, "src"), _Out(bufs, "mask"), _Out(bufs, "pos")
    if c.kind == "prefix":
        pstride = L if mutation == "stride_ignored" else c.stride
        poff = 0 if mutation == "offset_ignored" else c.offset
        for b in range(c.B):
            lds = [0] * S
            for s in range(S):
                if s < L:
                    sv, mv = -(1 + b * pstride + poff + s), 1
                else:
                    sv, mv = int(_rd(tok, t_off + b * T + s - L)), int(_rd(qm, q_off + b * T + s - L) != 0)
                src.put(src.off + b * S + s, _i32(sv))
                msk.put(msk.off + b * S + s, mv)
                lds[s] = mv
            _emulate_positions(lds, S, c.pos_mode, pos, pos.off + b * S, mutation)
        return
    n_img, status = c.n_img, _Out(bufs, "status")
    for b in range(c.B):
        lds = [0] * (2 * S + 64 * L)                      # (room for what a mutation writes past the row)
        for s in range(S):
            src.put(src.off + b * S + s, 0)
        carry = 0
        for t0 in range(0, T, 64):
            toks = [int(_rd(tok, t_off + b * T + t0 + lane)) if t0 + lane < T else 0 for lane in range(64)]
            is_s = [1 if (t0 + lane < T and SPECIAL - n_img < toks[lane] <= SPECIAL) else 0 for lane in range(64)]
            inc = [x + (0 if mutation == "sentinel_carry_dropped" else carry) for x in _iscan64(is_s)]
            for lane in range(64):
                t = t0 + lane
                if t >= T:
                    continue
                before = inc[lane] if mutation == "before_inclusive" else inc[lane] - is_s[lane]
                o = t + before * (L - 1)
                if is_s[lane]:
                    if before < n_img or mutation == "overfull_row_writes_its_extra_sentinel":
                        for l in range(L):
                            src.put(src.off + b * S + o + l, -(1 + (b * n_img + before) * L + l))
                            lds[o + l] = int(_rd(qm, q_off + b * T + t) != 0) if mutation == "slot_mask_from_question_mask" else 1
                elif o < S or mutation == "text_written_past_T_out":
                    src.put(src.off + b * S + o, _i32(toks[lane]))
                    lds[o] = int(_rd(qm, q_off + b * T + t) != 0)
            carry = inc[63]
        status.put(status.off + b, min(carry, n_img) if mutation == "status_capped_at_n_img" else carry)
        for s in range(S):
            msk.put(msk.off + b * S + s, lds[s])
        _emulate_positions(lds, S, c.pos_mode, pos, pos.off + b * S, mutation)


# ==================================================================================================================== labels
PAD, BOS = 2, 1
LABEL_ROWS = ("pad@0", "pad@63", "pad@64", "pad@T-1", "bos@63", "bos@64", "two-bos-before-the-pad", "bos-only-after-the-pad", "no-pad", "all-pad")


@dataclass(frozen=True)
class LabelsCase:
    name: str
    T: int
    L: int
    mode: int
    bos: int = BOS


def label_ids(c: LabelsCase):
    """(ids int64 [B, T], the LABEL_ROWS name of every row): the layouts that fit into T columns."""
    rng = _rng(f"labels-T{c.T}")
    T, rows, names = c.T, [], []
    for name in LABEL_ROWS:
        ids = rng.randint(3, TEXT_HI + 1, size=T).astype(np.int64)
        first_pad, bos_cols = None, []
        if name.startswith("pad@"):
            first_pad = T - 1 if name == "pad@T-1" else int(name[4:])
            if first_pad >= T:
                continue
            bos_cols = [first_pad // 2] if first_pad >= 1 else []
        elif name.startswith("bos@"):
            k = int(name[4:])
            if k >= T:
                continue
            bos_cols, first_pad = [k], (T - 1 if T - 1 > k + 1 else None)
        elif name == "two-bos-before-the-pad":
            if T < 5:
                continue
            bos_cols, first_pad = [0, 2], T - 2
        elif name == "bos-only-after-the-pad":
            if T < 3:
                continue
            first_pad = T // 2
        elif name == "no-pad":
            bos_cols = [1] if T > 1 else []
        elif name == "all-pad":
            ids[:] = PAD
        ids[bos_cols] = BOS
        if first_pad is not None:
            ids[first_pad] = PAD
            ids[first_pad + 3::3] = PAD                   # behind the first pad: text, further pads and one more BOS
            if first_pad + 2 < T:
                ids[first_pad + 2] = BOS
        rows.append(ids)
        names.append(name)
    return np.stack(rows), names


LABELS_T, LABELS_L = (1, 64, 65, 150), (0, 3, 70)
LABELS_CASES = [LabelsCase(f"labels-T{T}-L{L}-mode{m}", T, L, m) for T in LABELS_T for L in LABELS_L for m in (0, 1)]
LABELS_CASES += [LabelsCase(f"labels-T{T}-L3-mode0-nobos", T, 3, 0, bos=-1) for T in LABELS_T]


def ref_labels(ids, L: int, pad: int, bos: int, mode: int):
    """oracle.label_mask_vqa (mode 0) / oracle.label_mask_cc (mode 1) behind L columns of -100."""
    ids = torch.as_tensor(np.asarray(ids))
    lab = oracle.label_mask_vqa(ids, pad, bos) if mode == 0 else oracle.label_mask_cc(ids, pad)
    return torch.cat([torch.full((ids.shape[0], L), -100, dtype=torch.int64), lab], dim=1).numpy()


def materialize_labels(c: LabelsCase):
    ids, _ = label_ids(c)
    B = ids.shape[0]
    bufs = Bufs()
    bk, vw = window(B, c.T, c.T, torch.int64, elem_offset=1, fill=POISON_ID)
    vw.copy_(torch.from_numpy(ids))
    bufs.win["ids"] = (bk, vw)
    bufs.win["out"] = window(B, c.L + c.T, c.L + c.T, torch.int64, elem_offset=3, fill=POISON_I64)
    return bufs, {"ids": ids}


def check_labels(c: LabelsCase, ref, got: Bufs):
    bk, vw = got.win["out"]
    assert untouched(bk, vw, POISON_I64), f"{c.name}: labels were written outside their rows"
    g = _view_np(got.win["out"])
    assert np.array_equal(g, ref), f"{c.name}: {_first(g, ref)}"


LABEL_MUTATIONS = ("pad_carry_dropped", "bos_carry_dropped")


def emulate_labels(c: LabelsCase, bufs: Bufs, mutation: Optional[str] = None):
    ids, i_off = _in(bufs, "ids"), _geo(bufs, "ids")[0]
    out = _Out(bufs, "out")
    T, L, S, B = c.T, c.L, c.L + c.T, bufs.win["ids"][1].shape[0]
    for b in range(B):
        for s in range(L):
            out.put(out.off + b * S + s, -100)
        pad_seen = bos_seen = 0
        for t0 in range(0, T, 64):
            tok = [int(_rd(ids, i_off + b * T + t0 + lane)) if t0 + lane < T else PAD - 1 for lane in range(64)]
            is_pad = [1 if (t0 + lane < T and tok[lane] == PAD) else 0 for lane in range(64)]
            is_bos = [1 if (t0 + lane < T and tok[lane] == c.bos and not is_pad[lane]) else 0 for lane in range(64)]
            pad_inc = [x + (0 if mutation == "pad_carry_dropped" else pad_seen) for x in _iscan64(is_pad)]
            bos_inc = [x + (0 if mutation == "bos_carry_dropped" else bos_seen) for x in _iscan64(is_bos)]
            for lane in range(64):
                t = t0 + lane
                if t >= T:
                    continue
                if c.mode == 1:
                    lab = -100 if is_pad[lane] else tok[lane]
                elif pad_inc[lane] - is_pad[lane] == 0:
                    if is_pad[lane]:
                        lab = PAD
                    elif is_bos[lane]:
                        lab = -100
                    else:
                        lab = tok[lane] if bos_inc[lane] - is_bos[lane] > 0 else -100
                else:
                    lab = -100 if is_pad[lane] else tok[lane]
                out.put(out.off + b * S + L + t, lab)
            pad_seen, bos_seen = pad_inc[63], bos_inc[63]


# ===================================================================================================================== embed
EMBED_SOURCE = "fewshot-T65-L2-n3-pos1"        # src / pos of the embed cases: prefix and token rows interleave, OPT positions over masks with holes


@dataclass(frozen=True)
class EmbedCase:
    name: str
    E: int
    dtype: str
    wpe: bool

    def ld(self, operand: str) -> int:
        return self.E + 4 * (1 + ("wte", "prefix", "wpe", "x", "dx", "dprefix").index(operand))


EMBED_E = (4, 1020, 1024, 1028, 2560)
EMBED_CASES = [EmbedCase(f"embed-E{E}-{dt}-{'wpe' if w else 'nowpe'}", E, dt, w) for E in EMBED_E for dt in ("f32", "bf16") for w in (True, False)]


def ref_embed(src, pos, wte, prefix, wpe):
    """float64 [rows, E]: row r is wte[src[r]] (src >= 0) or prefix[-src[r] - 1], plus wpe[pos[r]] where a position table is given."""
    rows = []
    for r, sv in enumerate(src):
        sv = int(sv)
        e = wte[sv] if sv >= 0 else prefix[-sv - 1]
        rows.append(e.double() + wpe[int(pos[r])].double() if wpe is not None else e.double().clone())
    return torch.stack(rows)


def ref_embed_bwd(src, dx, n_prefix: int):
    """-> (d float64 [n_prefix, E], named bool [n_prefix]): d[-src[r] - 1] = dx[r] for every prefix row r names."""
    d = torch.zeros(n_prefix, dx.shape[1], dtype=torch.float64)
    named = torch.zeros(n_prefix, dtype=torch.bool)
    for r, sv in enumerate(src):
        sv = int(sv)
        if sv < 0:
            d[-sv - 1] = dx[r].double()
            named[-sv - 1] = True
    return d, named


_EMBED_ROWS = {}


def embed_rows():
    """(src, pos int64 [rows], number of prefix rows, rows of the position table) of EMBED_SOURCE, computed once."""
    if not _EMBED_ROWS:
        fc = next(c for c in FEWSHOT_CASES if c.name == EMBED_SOURCE)
        tokens, qmask, _ = row_inputs(fc)
        src, _, pos, _ = ref_fewshot_rows(tokens, qmask, fc.L, fc.n_img, SPECIAL, fc.pos_mode)
        _EMBED_ROWS.update(src=src.reshape(-1), pos=pos.reshape(-1), n_prefix=fc.B * fc.n_img * fc.L, n_pos=fc.S + 2)
    return _EMBED_ROWS


def _fill(bufs, nm, values, ld, dtype, fill=NAN, off=0):
    bk, vw = window(values.shape[0], values.shape[1], ld, dtype, elem_offset=off, fill=fill)
    vw.copy_(values)
    bufs.win[nm] = (bk, vw)


def materialize_embed(c: EmbedCase):
    R = embed_rows()
    rows, lim, dt = len(R["src"]), LIM[c.dtype], DT[c.dtype]
    v = {"src": R["src"], "pos": R["pos"], "wte": pattern(VOCAB, c.E, lim, 3, 5), "prefix": pattern(R["n_prefix"], c.E, lim, 5, 7, 1),
         "wpe": pattern(R["n_pos"], c.E, lim, 7, 11, 2) if c.wpe else None, "dx": pattern(rows, c.E, lim, 11, 13, 3)}
    bufs = Bufs()
    for nm in ("src", "pos"):
        bk, vw = window(1, rows, rows, torch.int32, elem_offset=4, fill=VOCAB - 1)       # (pads of the index lists stay inside the tables)
        vw.copy_(torch.from_numpy(R[nm])[None])
        bufs.win[nm] = (bk, vw)
    for nm in ("wte", "prefix") + (("wpe",) if c.wpe else ()):
        _fill(bufs, nm, v[nm], c.ld(nm), dt)
    _fill(bufs, "dx", v["dx"], c.ld("dx"), torch.float32)
    bufs.win["x"] = window(rows, c.E, c.ld("x"), torch.float32, fill=SENTINEL)
    bufs.win["dprefix"] = window(R["n_prefix"], c.E, c.ld("dprefix"), dt, fill=SENTINEL)
    return bufs, v


def reference_embed(c: EmbedCase, v):
    d, named = ref_embed_bwd(v["src"], v["dx"], embed_rows()["n_prefix"])
    return {"x": ref_embed(v["src"], v["pos"], v["wte"], v["prefix"], v["wpe"]), "d": d, "named": named}


def check_embed(c: EmbedCase, ref, got: Bufs):
    xb, xv = got.win["x"]
    assert untouched(xb, xv), f"{c.name}: x was written outside its window"
    assert not xv.isnan().any() and torch.equal(xv.double(), ref["x"]), f"{c.name}: x: {_first_diff(xv.double(), ref['x'])}"
    db, dv = got.win["dprefix"]
    assert untouched(db, dv), f"{c.name}: dprefix was written outside its window"
    named = ref["named"]
    assert 0 < int(named.sum()) < named.numel(), f"{c.name}: the case must name some prefix rows and leave some alone"
    assert not dv.isnan().any()
    assert torch.equal(dv.double()[named], ref["d"][named]), f"{c.name}: dprefix rows named by src: {_first_diff(dv.double()[named], ref['d'][named])}"
    rest = dv.double()[~named]
    assert torch.equal(rest, torch.full_like(rest, SENTINEL)), f"{c.name}: a prefix row that src does not name was written"


EMBED_MUTATIONS = ("bwd_second_pass_skipped", "bwd_writes_token_rows")


def emulate_embed(c: EmbedCase, bufs: Bufs, mutation: Optional[str] = None):
    """embed_assemble_kernel / embed_assemble_bwd_kernel: one block per row, 256 threads x 4 columns = 1024 columns a pass."""
    E = c.E
    src, pos = bufs.win["src"][1][0].tolist(), bufs.win["pos"][1][0].tolist()
    wte, prefix, dx = _in(bufs, "wte"), _in(bufs, "prefix"), _in(bufs, "dx")
    wpe = _in(bufs, "wpe") if c.wpe else None
    x, d = _Out(bufs, "x"), _Out(bufs, "dprefix")
    for row, sv in enumerate(src):
        e_base = sv * c.ld("wte") if sv >= 0 else (-sv - 1) * c.ld("prefix")
        table = wte if sv >= 0 else prefix
        for c0 in range(0, E, 1024):
            cols = np.arange(c0, min(c0 + 1024, E))
            val = _rd(table, e_base + cols)
            if wpe is not None:
                val = val + _rd(wpe, pos[row] * c.ld("wpe") + cols)
            x.put(x.off + row * x.ld + cols, val)
        if sv >= 0 and mutation != "bwd_writes_token_rows":
            continue
        drow = (-sv - 1) if sv < 0 else sv
        for c0 in range(0, E, 1024):
            if c0 and mutation == "bwd_second_pass_skipped":
                break
            cols = np.arange(c0, min(c0 + 1024, E))
            d.put(d.off + drow * d.ld + cols, _rd(dx, row * c.ld("dx") + cols))
    x.flush()
    d.flush()


# ====================================================================================================================== move
@dataclass(frozen=True)
class MoveCase:
    name: str
    dtype: str
    scatter: bool
    n: int
    cols: int

    @property
    def ld_src(self):
        return self.cols + (8 if self.dtype == "bf16" else 4)

    @property
    def ld_dst(self):
        return self.cols + (24 if self.dtype == "bf16" else 12)

    @property
    def other_rows(self):
        """Rows of the indexed side (gather: the source, scatter: the destination): more than n, so that some stay unnamed."""
        return self.n + 5


MOVE_COLS = {"bf16": (8, 2040, 2048, 2056), "f32": (4, 1020, 1024, 1028)}
MOVE_N = (1, 7, 300)
MOVE_CASES = [MoveCase(f"move-{'scatter' if sc else 'gather'}-{dt}-n{n}-c{cols}", dt, sc, n, cols)
              for dt in ("bf16", "f32") for cols in MOVE_COLS[dt] for n in MOVE_N for sc in (False, True)]
# (dtype, cols, ld_src, ld_dst, element offset of src, of dst) that eavqa_move_rows must refuse with EAVQA_E_ALIGN: 16-byte vectors
MOVE_REJECTED = (("bf16", 8, 16, 16, 1, 0), ("bf16", 8, 16, 16, 0, 4), ("bf16", 8, 12, 16, 0, 0), ("bf16", 8, 16, 20, 0, 0), ("bf16", 12, 16, 16, 0, 0),
                 ("f32", 4, 8, 8, 2, 0), ("f32", 4, 8, 8, 0, 1), ("f32", 4, 6, 8, 0, 0), ("f32", 4, 8, 10, 0, 0), ("f32", 6, 8, 8, 0, 0))


def move_accepts(dtype: str, cols: int, ld_src: int, ld_dst: int, src_off: int, dst_off: int) -> bool:
    """The alignment rule of eavqa_move_rows on 16-byte aligned backing buffers."""
    vec, es = (8, 2) if dtype == "bf16" else (4, 4)
    return not (cols % vec or ld_src % vec or ld_dst % vec or (src_off * es) % 16 or (dst_off * es) % 16)


def move_index(c: MoveCase):
    """int64 [n]: a slice of a permutation of the indexed side's rows; the gathers of more than one row repeat their first index."""
    idx = _rng(c.name).permutation(c.other_rows)[:c.n].astype(np.int64)
    if not c.scatter and c.n > 1:
        idx[-1] = idx[0]
    return idx


def ref_move_rows(src, idx, scatter: bool, dst_rows: int):
    """-> (dst float64 [dst_rows, cols], named bool [dst_rows]): dst[i] = src[idx[i]] (gather) or dst[idx[i]] = src[i] (scatter)."""
    dst = torch.zeros(dst_rows, src.shape[1], dtype=torch.float64)
    named = torch.zeros(dst_rows, dtype=torch.bool)
    for i, j in enumerate(idx):
        s, d = (i, int(j)) if scatter else (int(j), i)
        dst[d] = src[s].double()
        named[d] = True
    return dst, named


def materialize_move(c: MoveCase):
    src_rows, dst_rows = (c.n, c.other_rows) if c.scatter else (c.other_rows, c.n)
    v = {"src": pattern(src_rows, c.cols, LIM[c.dtype], 5, 3), "idx": move_index(c), "dst_rows": dst_rows}
    bufs = Bufs()
    _fill(bufs, "src", v["src"], c.ld_src, DT[c.dtype])
    bk, vw = window(1, c.n, c.n, torch.int32, elem_offset=4, fill=0)               # (pads of the index list stay inside both matrices)
    vw.copy_(torch.from_numpy(v["idx"])[None])
    bufs.win["idx"] = (bk, vw)
    bufs.win["dst"] = window(dst_rows, c.cols, c.ld_dst, DT[c.dtype], fill=SENTINEL)
    return bufs, v


def reference_move(c: MoveCase, v):
    return ref_move_rows(v["src"], v["idx"], c.scatter, v["dst_rows"])


def check_move(c: MoveCase, ref, got: Bufs):
    want, named = ref
    db, dv = got.win["dst"]
    assert untouched(db, dv), f"{c.name}: dst was written outside its window"
    assert not dv.isnan().any(), f"{c.name}: dst holds NaN"
    assert torch.equal(dv.double()[named], want[named]), f"{c.name}: {_first_diff(dv.double()[named], want[named])}"
    rest = dv.double()[~named]
    assert torch.equal(rest, torch.full_like(rest, SENTINEL)), f"{c.name}: a row of dst that idx does not name was written"
    if not c.scatter:
        assert bool(named.all())


MOVE_MUTATIONS = ("gather_and_scatter_swapped", "dst_stride_from_src")


def emulate_move(c: MoveCase, bufs: Bufs, mutation: Optional[str] = None):
    """move_rows_kernel: one block per index, 256 threads x one 16-byte vector a pass."""
    src, idx = _in(bufs, "src"), bufs.win["idx"][1][0].tolist()
    dst = _Out(bufs, "dst")
    scatter = c.scatter != (mutation == "gather_and_scatter_swapped")
    ldd = c.ld_src if mutation == "dst_stride_from_src" else c.ld_dst
    per_pass = 256 * (8 if c.dtype == "bf16" else 4)
    for i, j in enumerate(idx):
        s_row, d_row = (i, j) if scatter else (j, i)
        for c0 in range(0, c.cols, per_pass):
            cols = np.arange(c0, min(c0 + per_pass, c.cols))
            dst.put(dst.off + d_row * ldd + cols, _rd(src, s_row * c.ld_src + cols))
    dst.flush()


# ================================================================================================================= transpose
@dataclass(frozen=True)
class TransposeCase:
    name: str
    dtype: str
    rows: int
    cols: int
    src_off: int
    dst_off: int

    @property
    def ld_src(self):
        return self.cols + 4

    @property
    def ld_dst(self):
        return self.rows + 8

    @property
    def fast(self) -> bool:
        """The predicate of eavqa_transpose, on backing buffers that are 8-byte aligned: the 16-bit kernel moves 8-byte vectors."""
        sizes = self.rows | self.cols | self.ld_src | self.ld_dst
        return self.dtype == "bf16" and not (sizes & 3) and not ((2 * self.src_off | 2 * self.dst_off) & 7)


TRANSPOSE_SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (60, 68), (132, 68), (4, 260))
TRANSPOSE_OFFSETS = ((0, 0), (4, 0), (2, 0), (1, 0), (0, 4), (0, 2), (0, 1))
TRANSPOSE_CASES = [TransposeCase(f"transpose-{dt}-{r}x{cl}-src+{so}-dst+{do}", dt, r, cl, so, do)
                   for dt in ("f32", "bf16") for r, cl in TRANSPOSE_SHAPES for so, do in TRANSPOSE_OFFSETS]


def ref_transpose(x):
    xl = x.tolist()
    out = [[0.0] * x.shape[0] for _ in range(x.shape[1])]
    for r in range(x.shape[0]):
        for cl in range(x.shape[1]):
            out[cl][r] = xl[r][cl]
    return torch.tensor(out, dtype=torch.float64)


def materialize_transpose(c: TransposeCase):
    v = {"x": pattern(c.rows, c.cols, LIM[c.dtype], 3, 7)}
    bufs = Bufs()
    _fill(bufs, "src", v["x"], c.ld_src, DT[c.dtype], off=c.src_off)
    bufs.win["dst"] = window(c.cols, c.rows, c.ld_dst, DT[c.dtype], elem_offset=c.dst_off, fill=SENTINEL)
    return bufs, v


def check_transpose(c: TransposeCase, ref, got: Bufs):
    db, dv = got.win["dst"]
    assert untouched(db, dv), f"{c.name}: dst was written outside its window"
    assert not dv.isnan().any() and torch.equal(dv.double(), ref), f"{c.name}: {_first_diff(dv.double(), ref)}"


TRANSPOSE_MUTATIONS = ("edge_guard_tests_rows_against_cols", "fast_kernel_on_a_4_byte_aligned_pointer")


def emulate_transpose(c: TransposeCase, bufs: Bufs, mutation: Optional[str] = None):
    """transpose_kernel (one element a lane through a 64 x 64 tile) or transpose16_kernel (8-byte vectors: 4 columns of a row pair in,
    4 rows of a column out), chosen as eavqa_transpose does."""
    src, dst = _in(bufs, "src"), _Out(bufs, "dst")
    s_off, lds = _geo(bufs, "src")
    rows, cols, ldd = c.rows, c.cols, c.ld_dst
    fast, early = c.fast, 0
    if mutation == "fast_kernel_on_a_4_byte_aligned_pointer":
        sizes = rows | cols | c.ld_src | c.ld_dst
        fast = c.dtype == "bf16" and not (sizes & 3) and not ((2 * c.src_off | 2 * c.dst_off) & 3)
        early = 1 if fast and not c.fast else 0
    for r0 in range(0, rows, 64):
        for c0 in range(0, cols, 64):
            tile = np.zeros((64, 64))
            if fast:
                for rp in range(32):
                    for cq in range(16):
                        r, cl = r0 + 2 * rp, c0 + 4 * cq
                        if r < rows and cl < cols:
                            tile[2 * rp, 4 * cq:4 * cq + 4] = _rd(src, s_off - early + r * lds + cl + np.arange(4))
                            if r + 1 < rows:
                                tile[2 * rp + 1, 4 * cq:4 * cq + 4] = _rd(src, s_off - early + (r + 1) * lds + cl + np.arange(4))
                for cl in range(64):
                    for rq in range(16):
                        if c0 + cl < cols and r0 + 4 * rq < rows:
                            dst.put(dst.off + (c0 + cl) * ldd + r0 + 4 * rq + np.arange(4), tile[4 * rq:4 * rq + 4, cl])
                continue
            for i in range(64):
                tx = np.arange(64)
                ok = tx[(c0 + tx < cols)] if r0 + i < rows else tx[:0]
                tile[i, ok] = _rd(src, s_off + (r0 + i) * lds + c0 + ok)
            for i in range(64):
                tx = np.arange(64)
                if mutation == "edge_guard_tests_rows_against_cols":
                    ok = tx[r0 + tx < cols] if c0 + i < rows else tx[:0]
                else:
                    ok = tx[r0 + tx < rows] if c0 + i < cols else tx[:0]
                dst.put(dst.off + (c0 + i) * ldd + r0 + ok, tile[ok, i])
    dst.flush()


# ===================================================================================================================== gated
@dataclass(frozen=True)
class GatedCase:
    name: str
    dtype: str
    act: str
    rows: int
    F: int
    ldu: int
    ldh: int
    lddh: int
    lddu: int

    @property
    def exact(self):
        return self.act in EXACT_ACTS


GATED_SHAPES = ((1, 4, 8, 4, 4, 8), (37, 136, 280, 140, 144, 276), (520, 4100, 8204, 4104, 4100, 8200))
GATED_BLOCKS, GATED_THREADS = 2048, 256                # the launch cap of eavqa_gated_act_fwd / _bwd
GATED_TOL = {"f32": 1e-5, "bf16": 3e-2}                # test_gated_activation_forward_backward (tests/test_t5_gpu.py), of max(1, max |reference|)
GATED_CASES = [GatedCase(f"gated-{dt}-{act}-{s[0]}x{s[1]}", dt, act, *s) for s in GATED_SHAPES for dt in ("f32", "bf16") for act in EXACT_ACTS]
GATED_CASES += [GatedCase(f"gated-{dt}-{act}-{s[0]}x{s[1]}", dt, act, *s) for s in GATED_SHAPES[1:] for dt in ("f32", "bf16") for act in NONLINEAR]


def ref_gated_fwd(u, F: int, act: str):
    return ACT_F[act](u[:, :F]) * u[:, F:2 * F]


def ref_gated_bwd(u, dh, F: int, act: str):
    """du [rows, 2 F]: du[:, c] = dh u[:, F + c] act'(u[:, c]), du[:, F + c] = dh act(u[:, c])."""
    return torch.cat([dh * u[:, F:2 * F] * act_grad(act, u[:, :F]), dh * ACT_F[act](u[:, :F])], dim=1)


def materialize_gated(c: GatedCase):
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    if c.exact:            # |u| <= 8, |dh| <= 4: every product of the two passes is an integer of magnitude <= 64
        u = torch.randint(-8, 9, (c.rows, 2 * c.F), generator=g).double()
        dh = torch.randint(-4, 5, (c.rows, c.F), generator=g).double()
    else:
        u = (torch.rand(c.rows, 2 * c.F, generator=g) * 6 - 3).to(DT[c.dtype]).double()
        dh = (torch.rand(c.rows, c.F, generator=g) * 6 - 3).to(DT[c.dtype]).double()
    bufs = Bufs()
    _fill(bufs, "u", u, c.ldu, DT[c.dtype])
    _fill(bufs, "dh", dh, c.lddh, DT[c.dtype])
    bufs.win["h"] = window(c.rows, c.F, c.ldh, DT[c.dtype], fill=SENTINEL)
    bufs.win["du"] = window(c.rows, 2 * c.F, c.lddu, DT[c.dtype], fill=SENTINEL)
    return bufs, {"u": u, "dh": dh}


def reference_gated(c: GatedCase, v):
    return {"h": ref_gated_fwd(v["u"], c.F, c.act), "du": ref_gated_bwd(v["u"], v["dh"], c.F, c.act)}


WORST = {}          # (dtype, act, "h" | "du") -> worst error / bound of the real-valued legs seen by check_gated


def check_gated(c: GatedCase, ref, got: Bufs):
    for nm in ("h", "du"):
        bk, vw = got.win[nm]
        assert untouched(bk, vw), f"{c.name}: {nm} was written outside its window"
        g, want = vw.double(), ref[nm]
        assert not g.isnan().any(), f"{c.name}: {nm} holds NaN"
        if c.exact:
            assert torch.equal(g, want), f"{c.name}: {nm}: {_first_diff(g, want)}"
            continue
        bound = GATED_TOL[c.dtype] * max(1.0, want.abs().max().item())
        err = (g - want).abs()
        key = (c.dtype, c.act, nm)
        WORST[key] = max(WORST.get(key, 0.0), err.max().item() / bound)
        bad = ~(err <= bound)
        assert not bad.any(), (f"{c.name}: {nm}: {int(bad.sum())} elements beyond {bound:.3e}, first at {bad.nonzero()[0].tolist()}: "
                               f"|got - reference| = {err[tuple(bad.nonzero()[0].tolist())].item():.3e}")


GATED_MUTATIONS = ("second_pass_skipped", "gate_half_read_at_half_ldu", "du_halves_swapped")


def emulate_gated(c: GatedCase, bufs: Bufs, mutation: Optional[str] = None):
    """gated_act_fwd_kernel / gated_act_bwd_kernel: min(ceil(n4 / 256), 2048) blocks of 256 threads, 4 columns a thread, grid-stride passes."""
    u, dh = _in(bufs, "u"), _in(bufs, "dh")
    h, du = _Out(bufs, "h"), _Out(bufs, "du")
    F, q = c.F, c.F // 4
    n4 = c.rows * q
    stride = min((n4 + GATED_THREADS - 1) // GATED_THREADS, GATED_BLOCKS) * GATED_THREADS
    gate = c.ldu // 2 if mutation == "gate_half_read_at_half_ldu" else F
    rnd = (lambda x: x.to(DT[c.dtype]).double())
    for p0 in range(0, n4, stride):
        if p0 and mutation == "second_pass_skipped":
            break
        i = np.arange(p0, min(p0 + stride, n4))
        r, cl = i // q, (i % q) * 4
        idx = (r * c.ldu + cl)[:, None] + np.arange(4)[None, :]
        a, b = torch.from_numpy(_rd(u, idx)), torch.from_numpy(_rd(u, idx + gate))
        d = torch.from_numpy(_rd(dh, (r * c.lddh + cl)[:, None] + np.arange(4)[None, :]))
        h.put((r * c.ldh + cl)[:, None] + np.arange(4)[None, :], rnd(ACT_F[c.act](a) * b).numpy())
        lo, hi = rnd(d * b * act_grad(c.act, a)).numpy(), rnd(d * ACT_F[c.act](a)).numpy()
        if mutation == "du_halves_swapped":
            lo, hi = hi, lo
        o = (r * c.lddu + cl)[:, None] + np.arange(4)[None, :]
        du.put(o, lo)
        du.put(o + F, hi)
    h.flush()
    du.flush()


# ======================================================================================================================= vit
@dataclass(frozen=True)
class VitCase:
    name: str
    kind: str                       # patchify | assemble
    dtype: str
    B: int = 2
    img: int = 0                    # patchify
    ps: int = 0
    ldp: int = 0
    n_patch: int = 0                # assemble
    W: int = 0

    @property
    def ldpe(self):
        return self.W + 4

    @property
    def ldx(self):
        return self.W + 8


PATCHIFY_SHAPES = ((28, 14, 588), (28, 14, 608), (32, 16, 768))
VIT_W, VIT_NPATCH = (4, 1028, 1280), (1, 5)
VIT_CASES = [VitCase(f"patchify-{dt}-img{i}-ps{p}-ldp{l}", "patchify", dt, img=i, ps=p, ldp=l) for dt in ("f32", "bf16") for i, p, l in PATCHIFY_SHAPES]
VIT_CASES += [VitCase(f"vit-assemble-{dt}-W{W}-np{n}", "assemble", dt, n_patch=n, W=W) for dt in ("f32", "bf16") for W in VIT_W for n in VIT_NPATCH]


def ref_patchify(px, ps: int, ldp: int):
    """[B, 3, img, img] -> float64 [B g g, ldp]: patch (gy, gx) of image b is row (b g + gy) g + gx, its pixel (ch, i, j) column
    (ch ps + i) ps + j; the columns from 3 ps ps on are zero."""
    B, _, img, _ = px.shape
    g = img // ps
    out = torch.zeros(B * g * g, ldp, dtype=torch.float64)
    for b in range(B):
        for gy in range(g):
            for gx in range(g):
                for ch in range(3):
                    for i in range(ps):
                        col = (ch * ps + i) * ps
                        out[(b * g + gy) * g + gx, col:col + ps] = px[b, ch, gy * ps + i, gx * ps:(gx + 1) * ps].double()
    return out


def ref_vit_assemble(pe, cls, pos, B: int, n_patch: int):
    """float64 [B (n_patch + 1), W]: row (b, 0) = cls + pos[0], row (b, t) = pe[b n_patch + t - 1] + pos[t]."""
    rows = []
    for b in range(B):
        for t in range(n_patch + 1):
            rows.append((cls if t == 0 else pe[b * n_patch + t - 1]).double() + pos[t].double())
    return torch.stack(rows)


def materialize_vit(c: VitCase):
    lim, dt, bufs = LIM[c.dtype], DT[c.dtype], Bufs()
    if c.kind == "patchify":
        g = c.img // c.ps
        px = pattern(c.B * 3 * c.img, c.img, lim, 5, 3).reshape(c.B, 3, c.img, c.img)
        _fill(bufs, "px", px.reshape(1, -1), px.numel(), torch.float32, off=4)
        bufs.win["out"] = window(c.B * g * g, c.ldp, c.ldp, dt, elem_offset=4, fill=SENTINEL)
        return bufs, {"px": px}
    N = c.n_patch + 1
    v = {"pe": pattern(c.B * c.n_patch, c.W, lim, 3, 5), "cls": pattern(1, c.W, lim, 1, 7, 4), "pos": pattern(N, c.W, lim, 7, 3, 2)}
    _fill(bufs, "pe", v["pe"], c.ldpe, dt)
    _fill(bufs, "cls", v["cls"], c.W, torch.float32, off=4)
    _fill(bufs, "pos", v["pos"].reshape(1, -1), N * c.W, torch.float32, off=4)
    bufs.win["x"] = window(c.B * N, c.W, c.ldx, torch.float32, fill=SENTINEL)
    return bufs, v


def reference_vit(c: VitCase, v):
    if c.kind == "patchify":
        return ref_patchify(v["px"], c.ps, c.ldp)
    return ref_vit_assemble(v["pe"], v["cls"][0], v["pos"], c.B, c.n_patch)


def check_vit(c: VitCase, ref, got: Bufs):
    nm = "out" if c.kind == "patchify" else "x"
    bk, vw = got.win[nm]
    assert untouched(bk, vw), f"{c.name}: {nm} was written outside its window"
    assert not vw.isnan().any() and torch.equal(vw.double(), ref), f"{c.name}: {_first_diff(vw.double(), ref)}"


VIT_MUTATIONS = ("position_row_from_row", "patchify_pad_columns_not_zeroed")


def emulate_vit(c: VitCase, bufs: Bufs, mutation: Optional[str] = None):
    """patchify_kernel (one thread a pixel) + zero_cols_kernel; vit_assemble_kernel (one block a row, 1024 columns a pass)."""
    if c.kind == "patchify":
        px, p_off = _in(bufs, "px"), _geo(bufs, "px")[0]
        out = _Out(bufs, "out")
        img, ps, g = c.img, c.ps, c.img // c.ps
        idx = np.arange(c.B * 3 * img * img)
        x, t = idx % img, idx // img
        y, t2 = t % img, t // img
        ch, b = t2 % 3, t2 // 3
        gy, gx = y // ps, x // ps
        row = (b * g + gy) * g + gx
        col = (ch * ps + (y - gy * ps)) * ps + (x - gx * ps)
        out.put(out.off + row * c.ldp + col, _rd(px, p_off + idx))
        kreal = 3 * ps * ps
        if c.ldp > kreal and mutation != "patchify_pad_columns_not_zeroed":
            z = np.arange(c.B * g * g * (c.ldp - kreal))
            out.put(out.off + (z // (c.ldp - kreal)) * c.ldp + kreal + z % (c.ldp - kreal), 0.0)
        out.flush()
        return
    pe, cls, pos = _in(bufs, "pe"), _in(bufs, "cls"), _in(bufs, "pos")
    c_off, p_off = _geo(bufs, "cls")[0], _geo(bufs, "pos")[0]
    x = _Out(bufs, "x")
    N = c.n_patch + 1
    for row in range(c.B * N):
        b, t = row // N, row % N
        for c0 in range(0, c.W, 1024):
            cols = np.arange(c0, min(c0 + 1024, c.W))
            val = _rd(cls, c_off + cols) if t == 0 else _rd(pe, (b * c.n_patch + t - 1) * c.ldpe + cols)
            val = val + _rd(pos, p_off + (row if mutation == "position_row_from_row" else t) * c.W + cols)
            x.put(x.off + row * c.ldx + cols, val)
    x.flush()


GROUPS = {
    "fewshot": (FEWSHOT_CASES, materialize_rows, reference_rows, emulate_rows, check_rows),
    "prefix": (PREFIX_CASES, materialize_rows, reference_rows, emulate_rows, check_rows),
    "labels": (LABELS_CASES, materialize_labels, lambda c, v: ref_labels(v["ids"], c.L, PAD, c.bos, c.mode), emulate_labels, check_labels),
    "embed": (EMBED_CASES, materialize_embed, reference_embed, emulate_embed, check_embed),
    "move": (MOVE_CASES, materialize_move, reference_move, emulate_move, check_move),
    "transpose": (TRANSPOSE_CASES, materialize_transpose, lambda c, v: ref_transpose(v["x"]), emulate_transpose, check_transpose),
    "gated": (GATED_CASES, materialize_gated, reference_gated, emulate_gated, check_gated),
    "vit": (VIT_CASES, materialize_vit, reference_vit, emulate_vit, check_vit),
}
# mutation -> the groups whose emulation takes it
MUTATIONS = {m: ("prefix",) if m in ("stride_ignored", "offset_ignored") else ("fewshot", "prefix") if m.startswith("pos_") else ("fewshot",)
             for m in ROW_MUTATIONS}
for _ms, _g in ((LABEL_MUTATIONS, "labels"), (EMBED_MUTATIONS, "embed"), (MOVE_MUTATIONS, "move"), (TRANSPOSE_MUTATIONS, "transpose"),
                (GATED_MUTATIONS, "gated"), (VIT_MUTATIONS, "vit")):
    MUTATIONS.update({m: (_g,) for m in _ms})
