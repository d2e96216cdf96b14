"""Generates tests/golden/norm_bits.json: one SHA-256 per case of tests/_norm_bits.py, over the logical [rows, cols] region of every
output of the call, as the normalisation kernels compute it on the MI355X at the commit BEFORE they were restated as one row body per
pass and one host layer.  Run on the GPU in a tree of that commit with this file and tests/_norm_bits.py dropped in, the library built:

    python tests/golden/make_golden_norm_bits.py <commit id> [output path]

The commit id is an argument (the tree the recorder runs in need not be a git checkout) and is stored at the top of the file.  Every
case runs twice; a case whose two runs disagree, or that writes outside a window, stops the recording.  Data only: no program text."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def main(commit, path):
    import torch

    import _norm_bits as N
    from eavqa_amd import _lib, ops
    assert torch.cuda.is_available(), "record on the GPU"
    assert _lib.load().eavqa_check_device() == 0, "not a gfx950 device"
    digests = {}
    for name, c in N.CASES.items():
        (d1, bad1), (d2, bad2) = N.run(c, _lib.call, ops._stream()), N.run(c, _lib.call, ops._stream())
        assert not bad1 and not bad2, f"{name}: written outside the window of {bad1 or bad2}"
        assert d1 == d2, f"{name}: two runs disagree"
        digests[name] = d1
    with open(path, "w") as f:
        json.dump({"commit": commit, "device": torch.cuda.get_device_name(0), "cases": len(digests), "sha256": digests}, f, indent=0, sort_keys=False)
        f.write("\n")
    print(f"{path}: {len(digests)} cases recorded at {commit}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "norm_bits.json"))
