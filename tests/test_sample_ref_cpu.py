"""CPU: the sampling reference (tests/_sampling_ref.py) is HF's - its warpers against the installed transformers, its Philox against
Random123's known-answer vectors - and every fixed case of the GPU tests keeps its top-p boundary away from rounding."""
import numpy as np
import pytest
import torch

import _sampling_ref as R


def test_warpers_equal_transformers_on_the_gpu_cases():
    """Same finite mask and equal kept values as TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on every fixed case.
    (HF's top-p sums float32 probabilities; the cases keep the boundary 1e-4 away from every cumulative value, far beyond that.)"""
    lp = pytest.importorskip("transformers.generation.logits_process")
    logits = {(B, V): R.case_logits(B, V) for B, V, _ in R.SHAPES}
    n = 0
    for B, V, ld, t, k, p in R.filter_cases():
        x = logits[(B, V)]
        want = x.clone()
        if t != 1.0:
            want = lp.TemperatureLogitsWarper(t)(None, want)
        if k > 0:
            want = lp.TopKLogitsWarper(top_k=k)(None, want)
        if p < 1.0:
            want = lp.TopPLogitsWarper(top_p=p)(None, want)
        got = R.warp(x, t, k, p)
        assert torch.equal(torch.isfinite(got), torch.isfinite(want)), (B, V, t, k, p)
        keep = torch.isfinite(want)
        assert torch.equal(got[keep], want[keep]), (B, V, t, k, p)
        n += 1
    assert n == len(R.SHAPES) * len(R.TEMPERATURES) * len(R.TOP_KS) * len(R.TOP_PS)


def test_all_equal_row_keeps_every_token_under_top_k():
    """HF's tie rule (`scores < kth`): nothing is strictly below the third largest of equal values."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    x = torch.full((1, 64), 0.25)
    assert torch.isfinite(R.warp(x, 1.0, 3, 1.0)).all()
    assert torch.isfinite(lp.TopKLogitsWarper(top_k=3)(None, x.clone())).all()


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key) -> output."""
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for counter, key, want in kat:
        assert R.philox4x32_10(counter, key) == want
    u = R.philox_uniforms(7, 3, 5)
    assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all() and len(set(u.tolist())) == 5
    assert R.philox_uniform(0, 0, 0) == np.float32((0x6627e8d5 >> 8) * 2.0 ** -24)


def test_every_fixed_case_has_its_top_p_margin():
    """The condition under which the GPU tests ask for the exact mask with no case left out: no cumulative probability within 1e-4 of
    1 - top_p, by the reference alone."""
    logits = {(B, V): R.case_logits(B, V) for B, V, _ in R.SHAPES}
    for B, V, ld, t, k, p in R.filter_cases():
        assert R.top_p_margin(logits[(B, V)], t, k, p) >= 1e-4, (B, V, t, k, p)
    for (B, V), x in logits.items():
        finite = torch.isfinite(x)
        assert finite.any(dim=1).all() and not finite.all()                # some columns at -inf, never a whole row
        if V >= 1000:
            assert finite[:, V - 1].all() and finite[:, V - 1 - (V % 4096) // 2].all()      # the last column and the tail chunk hold mass


def test_inverse_cdf_and_margins():
    row = torch.tensor([0.0, R.NEG_INF, 0.0, 0.0, R.NEG_INF])
    assert [R.inverse_cdf(row, u) for u in (0.0, 0.3, 0.34, 0.7, 0.999)] == [0, 0, 2, 3, 3]
    assert R.inverse_cdf(row, 1.0) == 3                                    # rounding left none: the last token with mass
    assert abs(R.cdf_margin(row, 0.3) - (1 / 3 - 0.3)) < 1e-12
    assert abs(float(R.midpoint_uniform(row, 2)) - 0.5) < 1e-7
