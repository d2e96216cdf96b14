"""GPU: the full-sequence passes compute, bit for bit, what they computed before they were restated (one causal layer loop per route,
named tapes): tests/golden/lm_pass.npz holds the results of the cases of tests/_lm_pass_cases.py recorded twice, in two processes, by
tests/golden/make_golden_lm_pass.py at the commit before.  A quantity whose two recordings agree is asserted with ``array_equal`` (for one
above 4 KiB: the SHA-256 of its bytes); one stored twice (``...#2``: the recordings differ) must lie within twice the largest difference
between the two recordings - the route meant for the mapper's LayerNorm dgamma / dbeta, which ``ln_dparam_kernel`` sums with float
atomics.  On these shapes both recordings agree in every quantity, dgamma / dbeta included, so every assertion is an equality."""
import numpy as np
import pytest

from _lm_pass_cases import CASES, recorded
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOLERANCE_ROUTE = ("grad_ln_dgamma", "grad_ln_dbeta")        # the only quantities that may be stored twice


@pytest.fixture(scope="module")
def want():
    return load_golden("lm_pass.npz")


def test_the_fixture_covers_every_case_and_takes_the_tolerance_route_for_the_atomic_sums_only(want):
    assert {k.split("/")[0] for k in want} == {c.name for c in CASES}
    assert all(k[:-2].split("/")[1] in TOLERANCE_ROUTE for k in want if k.endswith("#2"))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_pass_results_equal_the_recording(case, want):
    import torch
    res = case.run(case.make("cuda"), "cuda")
    torch.cuda.synchronize()
    assert res
    for name, t in res.items():
        suffix, got = recorded(t)
        key = f"{case.name}/{name}{suffix}"
        a = want[key]
        if key + "#2" in want:
            b = want[key + "#2"]
            bound = 2.0 * np.abs(a.astype(np.float64) - b.astype(np.float64)).max()
            assert min(np.abs(got.astype(np.float64) - r.astype(np.float64)).max() for r in (a, b)) <= bound, key
        else:
            assert got.dtype == a.dtype and np.array_equal(got, a), key
