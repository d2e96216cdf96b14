"""GPU: ``eavqa_token_logprobs`` and ``eavqa_attention_merge`` (csrc/score.hip) with leading dimensions the wrappers in ``ops`` never pass,
through ctypes.  ``ops.token_logprobs`` always hands over tight label and output rows, ``ops.attention_merge`` the tensors' own strides,
which the other tests keep equal; here ``ld_labels`` and ``ld_out`` exceed ``n_labels``, and ``ld1``, ``ld2`` and ``ldo`` are three
different values.  Output pads hold a sentinel that must come back bit-unchanged; input pads hold values that would change the result
if a row were addressed with another stride."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _score_ref as ref

DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import _lib
    lib = _lib.load()
    assert lib.eavqa_check_device() == 0, "not a gfx950 device"
    return lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def test_token_logprobs_with_padded_label_and_output_rows(lib):
    """n_labels = 64 (the bound) in label rows of 70 and output rows of 67.  The label pads hold valid ids and the row behind the last
    one too, so a row addressed with ld = n_labels gathers other tokens; expected: the bits ``eavqa_logits_process(to_logprobs=1)``
    leaves, gathered (0 for the -100 pad and for an id >= V) - no tolerance."""
    from eavqa_amd import ops
    R, V, ld, n, ld_labels, ld_out = 5, 1000, 1004, 64, 70, 67
    g = torch.Generator().manual_seed(64)
    logits_h = torch.full((R, ld), math.nan)
    logits_h[:, :V] = 3.0 * torch.randn(R, V, generator=g)
    labels_h = torch.randint(0, V, (R + 1, ld_labels), generator=g)
    labels_h[0, 0], labels_h[1, n - 1], labels_h[2, 5], labels_h[3, 63], labels_h[4, 0] = -100, V, V - 1, 0, 10 ** 12
    out_h = torch.full((R + 1, ld_out), math.nan)
    logits, labels, out = logits_h.to(DEV), labels_h.to(DEV), out_h.to(DEV)
    rc = lib.eavqa_token_logprobs(R, V, ptr(logits), ld, ptr(labels), ld_labels, n, ptr(out), ld_out, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    lp = logits.clone()
    ops.logits_process(lp, V, None, 0, to_logprobs=True)
    lab = labels_h[:R, :n]
    ok = (lab >= 0) & (lab < V)
    want = torch.where(ok, lp[:, :V].cpu().gather(1, torch.where(ok, lab, torch.zeros_like(lab))), torch.zeros(()))
    got = out.cpu()
    assert torch.equal(got[:R, :n].view(torch.int32), want.view(torch.int32))
    assert bool((got[:R, :n][~ok] == 0).all()) and int((~ok).sum()) == 3 and bool((got[:R, :n][ok] < 0).all())
    pads = torch.ones(out_h.shape, dtype=torch.bool)
    pads[:R, :n] = False
    assert torch.equal(got[pads].view(torch.int32), out_h[pads].view(torch.int32))
    assert torch.equal(labels.cpu(), labels_h) and torch.equal(logits.cpu().view(torch.int32), logits_h.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_merge_with_three_different_leading_dimensions(lib, dtype):
    """Against the float64 two-segment formula (``lse_merge`` of tests/_score_ref.py) on the inputs as stored, within the bound of
    ``test_merge_of_prompt_and_candidate_segments_is_one_attention_over_all_keys``: 1e-5 in float32, 2^-7 of the largest expected
    element in bfloat16.  The input pads hold 1e4, the output buffer a sentinel in its pads and in one surplus row."""
    from eavqa_amd import _lib
    B, C, T, H, hd = 2, 3, 5, 3, 16
    E, rows = H * hd, B * C * T
    ld1, ld2, ldo = E + 8, E + 16, E + 24
    g = torch.Generator().manual_seed(7)

    def padded(ld, fill, n_rows=rows):
        x = torch.full((n_rows, ld), fill)
        x[:rows, :E] = torch.randn(rows, E, generator=g)
        return x.to(dtype)

    o1_h, o2_h, out_h = padded(ld1, 1.0e4), padded(ld2, 1.0e4), torch.full((rows + 1, ldo), 777.0).to(dtype)
    l1_h, l2_h = 2.0 * torch.randn(B, H, C * T, generator=g), 2.0 * torch.randn(B * C, H, T, generator=g)
    o1, o2, out, l1, l2 = (x.to(DEV) for x in (o1_h, o2_h, out_h, l1_h, l2_h))
    rc = lib.eavqa_attention_merge(_lib.F32 if dtype == torch.float32 else _lib.BF16, B, C, T, H, hd, ptr(o1), ld1, ptr(l1), ptr(o2), ld2, ptr(l2),
                                   ptr(out), ldo, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    # row r = (b C + c) T + t: l1[b, h, c T + t], l2[b C + c, h, t]
    w1 = l1_h.view(B, H, C, T).permute(0, 2, 3, 1).reshape(rows, H).double().numpy()
    w2 = l2_h.view(B * C, H, T).permute(0, 2, 1).reshape(rows, H).double().numpy()
    a, b = o1_h[:, :E].double().numpy().reshape(rows, H, hd), o2_h[:, :E].double().numpy().reshape(rows, H, hd)
    want = np.stack([ref.lse_merge(a[:, h], w1[:, h], b[:, h], w2[:, h]) for h in range(H)], axis=1).reshape(rows, E)
    got = out.cpu()
    err = np.abs(got[:rows, :E].double().numpy() - want).max()
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7 * np.abs(want).max()
    print(f"[{dtype}] merge with ld {ld1} / {ld2} / {ldo}: max |diff| {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    pads = torch.ones(out_h.shape, dtype=torch.bool)
    pads[:rows, :E] = False
    as_bits = lambda x: x.view(torch.int32 if dtype == torch.float32 else torch.int16)
    assert torch.equal(as_bits(got)[pads], as_bits(out_h)[pads])
    assert torch.equal(as_bits(o1.cpu()), as_bits(o1_h)) and torch.equal(as_bits(o2.cpu()), as_bits(o2_h))
