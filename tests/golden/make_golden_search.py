"""Generates tests/golden/search_modes.npz: what every generation mode of tests/_search_modes.py returns - ids, and scores where the
mode returns any - as THIS checkout computes them on the GPU.  It is a regression fixture, not a reference: record it at the commit whose
behaviour is to be kept, replay it (tests/test_search_modes_gpu.py) at the one that must not change it.

    python tests/golden/make_golden_search.py [output directory]

Per case the eos id is chosen so that the cut-off and the pad emission run: the case is first run with an eos id that is hardly ever generated, then recorded
with ``eos_token_id`` = a token some row generated second (or later, but not last) that is neither pad nor the config's eos, so that
row ends early while others may go on.  The ``rules`` cases keep the config's eos id: there the answer set ends the rows.  Every case is recorded twice; ``stable``
says whether the two recordings agree bit for bit (a case that does not is compared on its ids only).  The file holds data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _search_modes as sm  # noqa: E402


def pick_eos(name, free, banned):
    n_prompt = 1 if name.startswith("t5.") and ".prompt." not in name else 0         # T5 ids begin with the start token (a given prompt is cut off)
    for col in list(range(n_prompt + 1, free.shape[1] - 1)) + [n_prompt]:            # not the last column: the row has to end EARLY
        for t in free[:, col].tolist():
            if t not in banned:
                return int(t)
    raise RuntimeError(f"{name}: nothing but pad / eos was generated before the last position")


def same(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def record(out, name):
    cfg_eos, V = (sm.t5_model(name.split(".")[1]) if name.startswith("t5.") else sm.causal_model(name.split(".")[0]))[3:5]
    eos = cfg_eos
    if not name.endswith(".rules"):                                            # the free run: an eos id that is hardly ever generated
        eos = pick_eos(name, sm.run(name, V - 2)["ids"], {0, sm.CAUSAL_PAD, cfg_eos, V - 2})
    first, second = sm.run(name, eos), sm.run(name, eos)
    ids = first["ids"]
    early = [(row == eos).any() and int(np.argmax(row == eos)) < len(row) - 1 for row in ids]
    print(f"{name}: eos {eos}, ids {ids.shape}, rows that end early {sum(early)}/{len(early)}, stable {same(first, second)}")
    out[name] = dict(first, eos=eos, stable=same(first, second))


def main(out_dir):
    out = {}
    for name in sm.cases():
        record(out, name)
    path = os.path.join(out_dir, "search_modes.npz")
    np.savez_compressed(path, **sm.pack(out))
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
