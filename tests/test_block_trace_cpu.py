"""CPU: the kernel-call sequences of the decoder block drivers (csrc/lm_block.cpp, csrc/t5_block.cpp) are pinned.

The drivers are pure enqueue, so what they do is the list of kernel calls they make.  tests/block_trace/ compiles the two drivers together with
recording stubs of the twenty kernel entry points (the split plans stay the library's own) and prints every call of every case with all its
arguments; tests/golden/block_trace.txt is that output recorded from the drivers before they were folded onto one workspace layout and one
layer loop per route."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "block_trace.txt")


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    from eavqa_amd import build
    lib = build.build()
    exe = str(tmp_path_factory.mktemp("block_trace") / "block_trace")
    csrc, here = build.CSRC, os.path.join(ROOT, "tests", "block_trace")
    sources = [os.path.join(csrc, "lm_block.cpp"), os.path.join(csrc, "t5_block.cpp"), os.path.join(here, "stub.cpp"), os.path.join(here, "main.cpp")]
    cmd = [build._hipcc()] + build.FLAGS + [f"--offload-arch={build.ARCH}", "-x", "hip", f"-I{build.INCLUDE}", f"-I{csrc}"] + sources + \
          [f"-L{os.path.dirname(lib)}", "-leavqa_hip", f"-Wl,-rpath,{os.path.dirname(lib)}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _cases(text):
    """{case: (return code, workspace bytes, [call lines])} of a tracer output."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.fullmatch(r"== (\S+) rc=(-?\d+) ws=(\d+)", line)
        if m:
            cur = out[m.group(1)] = (int(m.group(2)), int(m.group(3)), [])
        else:
            cur[2].append(line)
    return out


def test_call_sequences_equal_the_recording(trace):
    with open(GOLDEN) as f:
        golden = "".join(line for line in f if not line.startswith("#"))
    got, want = _cases(trace), _cases(golden)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
    assert trace == golden


def test_every_workspace_pointer_lies_inside_the_workspace(trace):
    cases = _cases(trace)
    assert len(cases) == 21 and all(rc == 0 and calls for rc, _, calls in cases.values())
    for name, (_, ws, calls) in cases.items():
        offsets = [int(o) for line in calls for o in re.findall(r"ws\+(\d+)", line)]
        assert offsets and max(offsets) < ws, (name, max(offsets), ws)
