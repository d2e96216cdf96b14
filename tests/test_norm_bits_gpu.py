"""GPU: the normalisation kernels reproduce, bit for bit, what they computed before they were restated as one row body per pass
(tests/golden/norm_bits.json, recorded by tests/golden/make_golden_norm_bits.py at the commit named at its top; cases and inputs:
tests/_norm_bits.py).  Every recorded case must be present and equal, and nothing may be written outside an output's window."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

import _norm_bits as N

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert len(GOLDEN["commit"]) == 40
    assert set(GOLDEN["sha256"]) == set(N.CASES) and GOLDEN["cases"] == len(N.CASES)


@pytest.mark.parametrize("entry", N.ENTRIES)
def test_norm_bits_are_the_parents(entry):
    from eavqa_amd import _lib, ops
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    failed = []
    for name, c in N.CASES.items():
        if c["entry"] != entry:
            continue
        digest, outside = N.run(c, _lib.call, ops._stream())
        if outside:
            failed.append(f"{name}: written outside the window of {outside}")
        if digest != GOLDEN["sha256"][name]:
            failed.append(f"{name}: bits differ from commit {GOLDEN['commit'][:7]}")
    assert not failed, f"{len(failed)} cases:\n" + "\n".join(failed)
