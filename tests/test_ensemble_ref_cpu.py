"""CPU: tests/_ensemble_ref.py (what the GPU tests compare ``eavqa_ensemble_combine`` with) pinned to torch - product is the weighted
sum of ``log_softmax``, mixture is ``logsumexp(log_softmax + log w)`` over the members - on rows with and without -inf, and its weight
and -inf rules."""
import math

import pytest
import torch

import _ensemble_ref as ref

NEG_INF = float("-inf")


def _rows(B, n, V, seed, holes):
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(B * n, V, generator=g, dtype=torch.float64)
    if holes:
        x[torch.rand(B * n, V, generator=g) < 0.2] = NEG_INF
        x[:, 0] = 0.5                                          # every member keeps a finite column
    return x


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("n,weights", [(1, None), (2, None), (3, [0.2, 0.5, 0.3]), (4, [1.0, 2.0, 3.0, 2.0])])
def test_product_is_the_weighted_sum_of_log_softmax(n, weights, holes):
    x = _rows(3, n, 17, 11 * n, holes)
    w = torch.tensor(ref.normalise(weights, n), dtype=torch.float64)
    got = ref.combine(x, n, "product", weights)
    for b in range(3):
        want = (w[:, None] * torch.log_softmax(x[b * n:(b + 1) * n], dim=-1)).sum(0)
        assert torch.equal(torch.isinf(got[b]), torch.isinf(want))
        fin = ~torch.isinf(want)
        assert (got[b][fin] - want[fin]).abs().max().item() <= 1e-12
    assert not torch.isnan(got).any()


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("n,weights", [(1, None), (2, None), (3, [0.2, 0.5, 0.3]), (4, [1.0, 2.0, 3.0, 2.0])])
def test_mixture_is_logsumexp_of_log_softmax_plus_log_weight(n, weights, holes):
    x = _rows(3, n, 17, 7 * n, holes)
    w = torch.tensor(ref.normalise(weights, n), dtype=torch.float64)
    got = ref.combine(x, n, "mixture", weights)
    for b in range(3):
        want = torch.logsumexp(torch.log_softmax(x[b * n:(b + 1) * n], dim=-1) + torch.log(w)[:, None], dim=0)
        assert torch.equal(torch.isinf(got[b]), torch.isinf(want))
        fin = ~torch.isinf(want)
        assert (got[b][fin] - want[fin]).abs().max().item() <= 1e-12
        # a mixture of distributions is a distribution
        assert abs(torch.logsumexp(got[b], dim=0).item()) <= 1e-12
    assert not torch.isnan(got).any()


def test_minus_infinity_rules():
    x = _rows(1, 3, 9, 3, False)
    x[1, 4] = NEG_INF                                          # one member
    x[:, 6] = NEG_INF                                          # all members
    p, m = ref.combine(x, 3, "product"), ref.combine(x, 3, "mixture")
    assert p[0, 4] == NEG_INF and math.isfinite(m[0, 4])
    assert p[0, 6] == NEG_INF and m[0, 6] == NEG_INF
    assert not torch.isnan(p).any() and not torch.isnan(m).any()


@pytest.mark.parametrize("mode", ["product", "mixture"])
def test_a_member_of_weight_zero_does_not_count(mode):
    x = _rows(2, 3, 9, 5, False)
    x[0::3] = NEG_INF                                          # member 0: nothing finite
    x[2::3] = 1e4 * torch.sign(x[2::3])                        # member 2: huge
    got = ref.combine(x, 3, mode, [0.0, 4.0, 0.0])
    want = torch.log_softmax(x[1::3], dim=-1)
    assert not torch.isnan(got).any() and (got - want).abs().max().item() <= 1e-12


def test_weights_are_normalised_and_checked():
    assert ref.normalise(None, 4) == [0.25] * 4
    assert ref.normalise([2, 6], 2) == [0.25, 0.75]
    for bad in ([1.0, -0.1], [0.0, 0.0], [1.0], [float("nan"), 1.0], [float("inf"), 1.0]):
        with pytest.raises(ValueError):
            ref.normalise(bad, 2)


def test_member_lse_is_logsumexp():
    x = _rows(2, 2, 13, 9, True)
    _, lse = ref.member_logprobs(x)
    assert (lse - torch.logsumexp(x, dim=-1)).abs().max().item() <= 1e-12
