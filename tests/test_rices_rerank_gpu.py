"""GPU: RICES joint re-ranking (``eavqa_rices_joint_scores`` + ``utils/rices.py::rices_select``) against int64 / float64 numpy."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NDQ, NQI, NQ_MAX, K_MAX = 2500, 40, 70, 2048


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


def stable_desc(scores, n):
    """columns of the n largest entries per row: descending score, ties by the smaller column"""
    return np.argsort(-scores, axis=1, kind="stable")[:, :n]


@functools.lru_cache(maxsize=None)
def exact_problem(D, Ni):
    """Embeddings in {-1, 0, 1} (text: halves, so text similarities are multiples of 0.25): every sum is exact in fp32.  Train questions
    300 .. 1199 repeat questions 0 .. 299 three times over, text and image alike: long runs of exact ties in text_sim AND in joint."""
    r = np.random.RandomState(D * 1000 + Ni)
    tt = r.randint(-1, 2, (NDQ, D)).astype(np.float64) * 0.5
    q2img = r.randint(0, Ni, NDQ).astype(np.int32)
    tt[300:1200] = np.tile(tt[:300], (3, 1))
    q2img[300:1200] = np.tile(q2img[:300], 3)
    vt = r.randint(-1, 2, (NQ_MAX, D)).astype(np.float64) * 0.5
    ti = r.randint(-1, 2, (Ni, D)).astype(np.float64)
    vi = r.randint(-1, 2, (NQI, D)).astype(np.float64)
    qrow = r.randint(0, NQI, NQ_MAX).astype(np.int32)
    qrow[1::3] = qrow[0]                                            # several queries share an image row
    S = vt @ tt.T
    I = stable_desc(S, K_MAX)
    img = np.stack([ti[q2img[I[q]]] @ vi[qrow[q]] for q in range(NQ_MAX)])
    return dict(tt=tt, vt=vt, ti=ti, vi=vi, q2img=q2img, qrow=qrow, D=np.take_along_axis(S, I, 1), I=I, img=img)


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=DEV, dtype=dtype) if dtype is not None else t.to(DEV)


@pytest.mark.parametrize("Ni", [50, 900])
@pytest.mark.parametrize("D", [20, 512, 768])
@pytest.mark.parametrize("k", [1, 37, 256, 2048])
@pytest.mark.parametrize("Nq", [1, 3, 70])
def test_joint_scores_and_selection_exact(ops, Nq, k, D, Ni):
    from eavqa_amd.utils import rices
    p = exact_problem(D, Ni)
    text_sim, text_idx, img = p["D"][:Nq, :k], p["I"][:Nq, :k], p["img"][:Nq, :k]
    want = text_sim + img
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)      # exactly representable
    joint, img_sim = ops.rices_joint_scores(T(text_sim, torch.float32), T(text_idx), T(p["q2img"]), T(p["ti"], torch.float32),
                                            T(p["vi"], torch.float32), T(p["qrow"][:Nq]), want_img_sim=True)
    assert np.array_equal(joint.cpu().numpy().astype(np.float64), want)
    assert np.array_equal(img_sim.cpu().numpy().astype(np.float64), img)
    assert k == 1 or any(len(np.unique(w)) < k for w in want)                    # the ties are there
    for n in sorted({1, min(32, k), k}):
        cols = stable_desc(want, n)
        scores, rows = rices.rices_select(T(p["tt"], torch.float32), T(p["vt"][:Nq], torch.float32), T(p["ti"], torch.float32),
                                          T(p["vi"], torch.float32), T(p["q2img"]), T(p["qrow"][:Nq]), n=n, k=k, normalize=False,
                                          query_tile=32)
        assert scores.shape == rows.shape == (Nq, n) and rows.dtype == torch.int64
        assert np.array_equal(rows.cpu().numpy()[:, ::-1], np.take_along_axis(text_idx, cols, 1))
        assert np.array_equal(scores.cpu().numpy().astype(np.float64)[:, ::-1], np.take_along_axis(want, cols, 1))


@pytest.fixture(scope="module")
def real_problem():
    g = torch.Generator().manual_seed(11)
    Nq, k, D, Ni, Ndq, Nqi = 70, 2048, 768, 900, 5000, 30
    ti = torch.nn.functional.normalize(torch.randn(Ni, D, generator=g), dim=1)
    vi = torch.nn.functional.normalize(torch.randn(Nqi, D, generator=g), dim=1)
    text_sim = (0.3 + 0.6 * torch.rand(Nq, k, generator=g)).sort(dim=1, descending=True).values
    text_idx = torch.stack([torch.randperm(Ndq, generator=g)[:k] for _ in range(Nq)])
    q2img = torch.randint(0, Ni, (Ndq,), generator=g, dtype=torch.int32)
    qrow = torch.randint(0, Nqi, (Nq,), generator=g, dtype=torch.int32)
    j64 = text_sim.double() + torch.stack([ti[q2img[text_idx[q]].long()].double() @ vi[qrow[q]].double() for q in range(Nq)])
    return dict(ti=ti, vi=vi, text_sim=text_sim, text_idx=text_idx, q2img=q2img, qrow=qrow, j64=j64)


def test_joint_scores_real_valued(ops, real_problem):
    p = real_problem
    joint = ops.rices_joint_scores(*(p[n].to(DEV) for n in ("text_sim", "text_idx", "q2img", "ti", "vi", "qrow")))
    j64 = p["j64"]
    err = (joint.cpu().double() - j64).abs().max().item()
    print(f"joint scores: max |d| against float64 = {err:.3e}")
    assert err <= 2e-5, err
    n = 32
    top, col = ops.topk_rows(joint, n)
    s64, c64 = torch.sort(j64, dim=1, descending=True, stable=True)
    assert (top.cpu().double() - s64[:, :n]).abs().max().item() <= 2e-5
    gap = s64[:, :n] - s64[:, 1:n + 1]                                  # rank r against rank r + 1 (the 33rd included)
    clear = gap > 4e-5
    clear[:, 1:] &= gap[:, :-1] > 4e-5
    print(f"joint selection: {clear.float().mean().item():.3f} of the ranks are clear in float64")
    assert clear.float().mean().item() >= 0.9
    assert bool((col.cpu()[clear] == c64[:, :n][clear]).all())
    again = ops.rices_joint_scores(*(p[n].to(DEV) for n in ("text_sim", "text_idx", "q2img", "ti", "vi", "qrow")))
    assert torch.equal(again, joint)                                    # fixed summation order


def test_joint_scores_guards(ops, real_problem):
    from eavqa_amd import _lib
    p = real_problem
    Ndq, Ni, Nqi = p["q2img"].numel(), p["ti"].shape[0], p["vi"].shape[0]
    args = {n: p[n].clone().to(DEV) for n in ("text_sim", "text_idx", "q2img", "ti", "vi", "qrow")}
    clean = ops.rices_joint_scores(*args.values())
    args["text_idx"][3, 5] = Ndq
    args["text_idx"][4, 0] = -1
    victim = int(args["text_idx"][6, 2])
    args["q2img"][victim] = Ni
    args["qrow"][9] = Nqi
    joint, img_sim = ops.rices_joint_scores(*args.values(), want_img_sim=True)      # returns EAVQA_OK (ops raises otherwise)
    bad = torch.zeros_like(clean, dtype=torch.bool)
    bad[3, 5] = bad[4, 0] = True
    bad[9, :] = True
    bad |= args["text_idx"] == victim
    assert bool(bad[6, 2])
    assert bool(torch.isneginf(joint[bad]).all()) and bool(torch.isneginf(img_sim[bad]).all())
    assert torch.equal(joint[~bad], clean[~bad])
    top, col = ops.topk_rows(joint, 2048)
    finite = torch.isfinite(top)
    assert bool((finite[:, 1:] <= finite[:, :-1]).all())                # nothing is selected ahead of a finite score
    assert bool(finite[:9].sum(1).eq(2048 - bad[:9].sum(1)).all()) and not bool(finite[9].any())

    lib = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ts, tix, q2, ti, vi, qr = (args[n] for n in ("text_sim", "text_idx", "q2img", "ti", "vi", "qrow"))
    out = torch.empty_like(ts)

    def raw(k=2048, D=768, ti_ptr=None, ld=768):
        return lib.eavqa_rices_joint_scores(70, k, D, Ndq, Ni, Nqi, ptr(ts), ptr(tix), ptr(q2), ti_ptr or ptr(ti), ld, ptr(vi), ld, ptr(qr),
                                            ptr(out), None, None)

    assert raw(D=22, ld=24) == -3                                       # EAVQA_E_SHAPE: D % 4
    assert raw(ti_ptr=ctypes.c_void_p(ti.data_ptr() + 4)) == -2         # EAVQA_E_ALIGN: rows not 16-byte aligned
    assert raw(ld=770) == -2
    assert raw(k=4096) == -3                                            # EAVQA_E_SHAPE: k > 2048
    assert lib.eavqa_rices_joint_scores(70, 2048, 768, Ndq, Ni, Nqi, ptr(ts), None, ptr(q2), ptr(ti), 768, ptr(vi), 768, ptr(qr), ptr(out),
                                        None, None) == -1
    assert raw(k=0) == -1


def test_question_only_is_the_text_neighbours_reversed(ops):
    from eavqa_amd.utils import rices
    g = torch.Generator().manual_seed(2)
    tt, vt = torch.randn(3000, 512, generator=g).to(DEV), torch.randn(50, 512, generator=g).to(DEV)
    D, I = rices.knn_inner_product(tt, vt, k=256)
    scores, rows = rices.rices_select(tt, vt, None, None, None, None, n=32, k=256, question_only=True)
    assert torch.equal(rows, I[:, :32].flip(1)) and torch.equal(scores, D[:, :32].flip(1))
