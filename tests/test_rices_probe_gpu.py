"""GPU: exact one-hot probes for ``eavqa_rices_joint_scores`` (csrc/retrieval.hip, ``joint_scores_kernel<NC>``).

The cases and the reference are tests/_answer_probe.py (what each case is and why its sums are exact: there and in
tests/test_answer_probe_cpu.py).  Calls go through ctypes, so every leading dimension is the case's own: ``joint`` and ``img_sim`` are
``[Nq + 1, k]`` buffers full of NaN whose surplus row must come back bit-unchanged, every round of a case runs twice (bit-equal) and a
third time with ``img_sim = NULL``, in the contiguous and in the window layout (``ld_train = D + 4``, ``ld_query = D + 12``, pads and a
surplus row of 3e4), and every input is bit-unchanged afterwards.  Results are compared with ``array_equal``: no tolerance.

Which case enters which path (ids are ``test_joint_cases[D..-k..-Nq..-kind]``; <2> and <3> are D = 512 / 768 of
tests/test_rices_rerank_gpu.py), and the mutation that turns it red ("run" = built into a scratch copy of the library and run once on
the MI355X, result stated; "read" = argued from the code):
  joint_scores_kernel<1>          D256-*      `s < NC` -> `s < NC - 1` in the dot-product loop (run: all 40 cases of D256 and D1024
  joint_scores_kernel<4>          D1024-*     red, the 84 others green)
  joint_scores_kernel<0>, a second 256-column step taken by lane 0 alone (D260), full and ragged steps (D516, D1028), a multiple of 256
  above 1024 (D1280), 64 steps (D16384)
                                  D260-* .. D16384-*      `c += 256` -> one step (`if (c < D)`) in the generic loop (run: all 84 cases
                                  of D260, D516, D1028, D1280 and D16384 red, the 40 of D256 / D1024 green)
  ld_train > D, ld_query > D      every case, window layout       `ld_train` -> `D` in `rows[r]` (run: all 124 cases red, every one
                                  of them at its first window round, after its contiguous rounds had passed).  A first version of
                                  the cases let neighbour 0 of query 0 be train row 0, whose address no stride enters: that run
                                  left the 12 k1-Nq1 cases green, so the neighbour lists now start at train row 3.
                                  `ld_query` -> `D` in `qrow`: every case's reference changes (read; tests/test_answer_probe_cpu.py)
  query row staged in LDS / qv[]  *-train_onehot: a dense query row against one element per train row; `query_row[i]` -> row 0
                                  changes every case whose query 0 is not row 0 (read)
  D = 16384: 65 536 bytes of dynamic LDS      D16384-k9-*: the launch succeeds on gfx950 (64 KB is within the workgroup's limit)
  k at the workgroup edge         *-k127-*, *-k128-*, *-k129-*: one workgroup of 127 / 128 neighbours, a second one holding 1; the RJ
                                  tail: k = 129 and 5 (RJ = 4: D256, D1024; RJ = 8: the others), `j0 + lane < j_end`.  Dropping the
                                  guard writes past joint[Nq, k] (moves an address: read, not run) - the NaN surplus row is what
                                  would show it.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _answer_probe as P

DEV = "cuda"
NAN_BITS = np.float32(math.nan).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import _lib
    lib = _lib.load()
    assert lib.eavqa_check_device() == 0, "not a gfx950 device"
    return lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _launch(lib, c, dev, lds, want_img):
    """one call into NaN-filled [Nq + 1, k] buffers; returns (joint, img_sim or None) [Nq, k] after checking the surplus row"""
    joint = torch.full((c.Nq + 1, c.k), math.nan, device=DEV)
    img = torch.full((c.Nq + 1, c.k), math.nan, device=DEV) if want_img else None
    rc = lib.eavqa_rices_joint_scores(c.Nq, c.k, c.D, c.Ndq, c.Ni, c.Nqi, ptr(dev["text_sim"]), ptr(dev["text_idx"]), ptr(dev["q2img"]),
                                      ptr(dev["train"]), lds[0], ptr(dev["query"]), lds[1], ptr(dev["query_row"]), ptr(joint),
                                      ptr(img) if want_img else None, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = []
    for t in (joint, img):
        if t is None:
            out.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[c.Nq].view(np.uint32) == NAN_BITS).all(), "the row behind the last query was written"
        out.append(h[:c.Nq])
    return out


@pytest.mark.parametrize("name", [c.name for c in P.joint_cases()])
def test_joint_cases(lib, name):
    c = P.joint_case(name)
    fixed = {n: getattr(c, n) for n in ("text_sim", "text_idx", "q2img")}
    for layout in P.JS_LAYOUTS:
        lds = P.js_lds(c.D, layout)
        dev = {n: torch.from_numpy(a).to(DEV) for n, a in fixed.items()}
        held = {}                                               # id(table) -> (host window, device copy): uploaded once, checked at the end
        for t in range(c.n_rounds):
            train, query, query_row, _ = c.round(t)
            for n, table, ld in (("train", train, lds[0]), ("query", query, lds[1])):
                if id(table) not in held:
                    w = P.window(table, ld)
                    held[id(table)] = (w, torch.from_numpy(w).to(DEV), table)
                dev[n] = held[id(table)][1]
            dev["query_row"] = torch.from_numpy(query_row).to(DEV)
            want_joint, want_img = P.joint_reference(c, t, layout, bufs=(held[id(train)][0], held[id(query)][0]))
            assert np.abs(want_joint).max() < 2 ** 23
            joint, img = _launch(lib, c, dev, lds, True)
            where = (layout, t)
            assert np.array_equal(img.astype(np.float64), want_img), where
            assert np.array_equal(joint.astype(np.float64), want_joint), where
            joint2, img2 = _launch(lib, c, dev, lds, True)
            assert np.array_equal(_bits(joint2), _bits(joint)) and np.array_equal(_bits(img2), _bits(img)), where
            joint3, _ = _launch(lib, c, dev, lds, False)
            assert np.array_equal(_bits(joint3), _bits(joint)), where
            assert np.array_equal(dev["query_row"].cpu().numpy(), query_row), where
        for w, d, _ in held.values():
            assert np.array_equal(_bits(d.cpu().numpy()), _bits(w)), layout
        for n, a in fixed.items():
            assert np.array_equal(_bits(dev[n].cpu().numpy()), _bits(a)), (layout, n)
