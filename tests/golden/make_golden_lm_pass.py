"""Generates tests/golden/lm_pass.npz: what the full-sequence passes of tests/_lm_pass_cases.py compute on the MI355X, recorded from the
commit BEFORE the Python passes were restated (one causal layer loop, named tapes), so that the restated passes are held to the same bits.
Run on the GPU at that commit, twice, in two processes, then merge:

    python tests/golden/make_golden_lm_pass.py record /tmp/a.npz
    python tests/golden/make_golden_lm_pass.py record /tmp/b.npz
    python tests/golden/make_golden_lm_pass.py merge /tmp/a.npz /tmp/b.npz

Per case the file holds every tensor the case returns (loss, count, logits, the gradient w.r.t. the prefix / encoder rows, the mapper's
flat gradient, the [B, C, Tc] token log-probabilities) under ``<case>/<quantity>``; a quantity above 4 KiB is held as the SHA-256 of its
bytes (``<case>/<quantity>@sha256``).  A quantity whose two recordings agree bit for bit is stored once and asserted with ``array_equal``;
one that does not is stored twice (``...`` and ``...#2``) and ``merge`` prints it: the test then takes the tolerance route, which is
meant for the mapper's LayerNorm dgamma / dbeta (float atomics) only.  Data only: no program text.

The Llama cases and the ``*_cached`` cases (prefill + two cached steps of every family) were recorded the same way from commit 09957cd,
the commit before the Llama family was folded into the one layer loop; the arrays of the 49 earlier cases came out byte for byte as
committed, and every quantity of the 20 new cases agreed between the two recordings."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def record(path):
    import torch

    from _lm_pass_cases import CASES, recorded
    assert torch.cuda.is_available(), "record on the GPU"
    out = {}
    for case in CASES:
        res = case.run(case.make("cuda"), "cuda")
        torch.cuda.synchronize()
        for name, t in res.items():
            suffix, a = recorded(t)
            out[f"{case.name}/{name}{suffix}"] = a
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} quantities of {len(CASES)} cases")


def merge(a_path, b_path):
    with np.load(a_path) as a, np.load(b_path) as b:
        assert sorted(a.files) == sorted(b.files)
        out = {}
        for k in a.files:
            out[k] = a[k]
            if a[k].tobytes() != b[k].tobytes():
                out[k + "#2"] = b[k]
                diff = "digest" if k.endswith("@sha256") else f"max |a - b| {np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max():.3e}"
                print(f"not reproduced between the two recordings: {k} ({diff})")
    dst = os.path.join(HERE, "lm_pass.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(out)} arrays, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "merge":
        merge(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
