"""GPU: every generation mode returns what the commit that recorded tests/golden/search_modes.npz returned, bit for bit - ids, and
scores where the mode returns any.  The grid (tests/_search_modes.py): both LM families in fp32 on the tiny committed weights, B = 3,
``max_length`` = 6, an eos id that some row emits early (so the pad emission and the cut-off run); every step source of the pick loop
(T5: native cached steps, the same calls from Python, re-forward, a 2-token left-padded decoder prompt; causal: per-row cache, shared
prompt cache, re-forward on single and on replicated rows) under greedy search, one draw and three draws per item; each plain, with
``repetition_penalty`` plus ``allowed_sequences``, and with ``output_scores``; and one 2-beam call per family, cached and not.

Exact equality is derived, not measured: the decoding loops were re-arranged, not their arithmetic - the same kernels run on the same
inputs in the same order.  The fixture was recorded twice, in two processes;
all 126 cases agreed bit for bit, within a process and between the two (``stable`` is True for each; a case for which it were False
would be compared on its ids only)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _search_modes as sm
from conftest import load_golden

FIXTURE = sm.unpack(load_golden("search_modes.npz"))


def test_the_fixture_holds_the_whole_grid():
    assert list(FIXTURE) == list(sm.cases())
    assert all(f["stable"] for f in FIXTURE.values())


@pytest.mark.parametrize("name", list(sm.cases()))
def test_mode_returns_what_the_recording_commit_returned(name):
    want = FIXTURE[name]
    got = sm.run(name, want["eos"])
    assert got["ids"].shape == want["ids"].shape and np.array_equal(got["ids"], want["ids"]), (got["ids"], want["ids"])
    assert ("scores" in got) == ("scores" in want)
    if "scores" in want and want["stable"]:
        assert got["scores"].dtype == np.float32 and got["scores"].shape == want["scores"].shape
        assert np.array_equal(got["scores"], want["scores"]), float(np.nanmax(np.abs(got["scores"] - want["scores"])))
