"""CPU: the beam-search entry points validate their arguments before any launch, the reference fixture is in place with its recorded
ranking margins, and ``VCT0Model.generate`` names the generation arguments it does not build."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


P = 4096      # a non-null, 16-byte aligned value standing in for a device pointer: every call below must return before it is used


def _beam_step(lib, B=2, k=2, V=32, ld=32, cur_len=1, max_length=8, ptrs=None, ws=P, ws_bytes=1 << 20):
    ptrs = [P] * 11 if ptrs is None else ptrs
    return lib.eavqa_beam_step(B, k, V, ptrs[0], ld, cur_len, max_length, 1, 1.0, 1.0, 0, *ptrs[1:], ws, ws_bytes, None)


def test_beam_step_rejects_bad_arguments_before_any_launch(lib):
    for i in range(11):                                            # every pointer, and the workspace
        assert _beam_step(lib, ptrs=[None if j == i else P for j in range(11)]) == -1
    assert _beam_step(lib, ws=None) == -1
    assert _beam_step(lib, k=9) == -3 and _beam_step(lib, k=0) == -3 and _beam_step(lib, k=-1) == -3
    assert _beam_step(lib, V=33, ld=32) == -3                      # V > ld
    assert _beam_step(lib, k=8, V=15, ld=16) == -3                 # fewer than 2k candidates per row
    assert _beam_step(lib, cur_len=8) == -1 and _beam_step(lib, cur_len=0) == -1 and _beam_step(lib, B=0) == -1
    need = lib.eavqa_beam_step_workspace_bytes(2, 2)
    assert need == 2 * 2 * 4 * 8 + 16 and _beam_step(lib, ws_bytes=need - 1) == -1
    assert lib.eavqa_beam_step_workspace_bytes(2, 9) == 0 and lib.eavqa_beam_step_workspace_bytes(0, 2) == 0


def test_beam_reorder_rejects_bad_arguments_before_any_launch(lib):
    ok = dict(dtype=1, n_planes=4, rows=6, t=3, t_max=7, inner=64, src=P, dst=2 * P, stride=6 * 7 * 64, parents=P)

    def call(**kw):
        a = {**ok, **kw}
        return lib.eavqa_beam_reorder(a["dtype"], a["n_planes"], a["rows"], a["t"], a["t_max"], a["inner"], a["src"], a["dst"], a["stride"], a["parents"], None)

    assert call(src=None) == -1 and call(dst=None) == -1 and call(parents=None) == -1
    assert call(dst=P) == -1                                        # in place: a gather must not overwrite its own sources
    assert call(dtype=7) == -4 and call(dtype=2) == -4
    assert call(t=8) == -1 and call(t=0) == -1 and call(stride=6 * 7 * 64 - 1) == -1
    assert call(inner=12, stride=6 * 7 * 12) == -2                  # bf16 rows of 24 bytes: not a multiple of 16
    assert call(src=P + 8) == -2


def test_beams_decoder_step_rejects_bad_arguments_before_any_launch(lib):
    from eavqa_amd import _lib
    table = (_lib.T5DecLayer * 1)()
    ws = lib.eavqa_t5_decoder_step_beams_workspace_bytes

    def call(dtype=1, layers=table, beams=3, x=P, workspace=P, nbytes=None, H=4):
        nbytes = ws(dtype, 2, beams, 64, 64, 128, 1) if nbytes is None else nbytes
        return lib.eavqa_t5_decoder_step_beams(dtype, 1, layers, P, 64, 64, H, 128, 1, 3, 1e-6, 2, beams, 2, 8, 5, x, P, None, 0, P, 15, 7, workspace, nbytes, None)

    assert call(layers=None) == -1 and call(x=None) == -1 and call(workspace=None) == -1
    assert call(dtype=7) == -4
    assert call(beams=9) == -3 and call(beams=0) == -3 and call(H=5) == -3
    assert call(nbytes=ws(1, 2, 3, 64, 64, 128, 1) - 1) == -1       # the size it checks is the size it uses
    assert ws(1, 2, 3, 64, 64, 128, 1) == ws(1, 6, 1, 64, 64, 128, 1) and ws(0, 2, 3, 64, 64, 128, 1) > ws(1, 2, 3, 64, 64, 128, 1)


def _fixture_flags(z, tag, name):
    """What a committed case exercises, recomputed from its arrays: ``moved`` - a returned hypothesis changed beam slot at a step >= 1 (a
    parent vector that is not the identity: the K / V reorder matters); ``short`` - a returned hypothesis shorter than max_length - 1
    beside one of full length (one entered the pool by eos and stayed); ``differs`` - the best beam is not what greedy search returns."""
    f = lambda field: z[f"{tag}.{name}.{field}"]
    k, nrs, es, eos, max_length = [int(v) for v in f("params")]
    bi, seq, greedy = f("beam_indices").astype(np.int64), f("sequences"), f("greedy")
    B = bi.shape[0] // nrs
    hist = bi - (np.repeat(np.arange(B), nrs) * k)[:, None]
    moved = bool(((hist[:, 2:] != hist[:, 1:-1]) & (bi[:, 2:] >= 0)).any())
    lens = (bi >= 0).sum(1)
    short = bool((lens < max_length - 1).any() and (lens == max_length - 1).any())
    # a short hypothesis ends with eos and is filled with eos (HF's fill value `pad or eos` with T5's pad id 0)
    for row, n in zip(seq, lens):
        assert n == max_length - 1 or (row[n] == eos and (row[n:] == eos).all()), (tag, name)
    best = seq.reshape(B, nrs, -1)[:, 0]
    n = min(best.shape[1], greedy.shape[1])
    differs = best.shape[1] != greedy.shape[1] or not np.array_equal(best[:, :n], greedy[:, :n])
    return moved, short, differs


def test_beam_fixture_exercises_what_its_generator_requires():
    """tests/golden/make_golden_beam.py: the three few-shot settings have a parent move and a short hypothesis beside a full-length one on
    both models, except (k = 4, length_penalty 2) on t5v10, where no seed and no eos id gives a short hypothesis (its docstring);
    per model at least one best beam differs from greedy search."""
    z = load_golden("vct0_beam.npz")
    for tag in ("t0", "t5v10"):
        flags = {name: _fixture_flags(z, tag, name) for name in z["cases"].tolist()}
        for name in ("fs_k3", "fs_k4_lp2", "fs_k2_es"):
            moved, short, _ = flags[name]
            assert moved, (tag, name)
            assert short or (tag, name) == ("t5v10", "fs_k4_lp2"), (tag, name)
        assert any(d for _, _, d in flags.values()), tag
        # the four other cases: the generator prefers both conditions; what the committed file holds
        assert sum(m and s for m, s, _ in flags.values()) >= 5, (tag, flags)


def test_beam_fixture_is_present_with_its_margins():
    z = load_golden("vct0_beam.npz")
    cases = z["cases"].tolist()
    assert len(cases) == 7 and set(z["paths"].tolist()) == {"fs", "prefix", "text"}
    for tag in ("t0", "t5v10"):
        for name in cases:
            assert float(z[f"{tag}.{name}.min_gap"]) >= 1e-3, (tag, name)
            k, nrs, es, eos, max_length = [int(v) for v in z[f"{tag}.{name}.params"]]
            seq = z[f"{tag}.{name}.sequences"]
            assert seq.shape[0] == 3 * nrs and seq.shape[1] <= max_length and eos > 1 and 1 <= nrs <= k <= 8
            assert z[f"{tag}.{name}.sequences_scores"].shape == (3 * nrs,)


def test_generation_arguments_that_are_not_built_are_named():
    from eavqa_amd.models.vct0 import generation_plan
    with pytest.raises(NotImplementedError, match="do_sample"):
        generation_plan(dict(num_beams=2, do_sample=True))
    with pytest.raises(NotImplementedError, match="decoder_input_ids"):
        generation_plan(dict(num_beams=2), decoder_input_ids=object())
    with pytest.raises(NotImplementedError, match="eos_token_id"):
        generation_plan(dict(num_beams=2, eos_token_id=[1, 2]))
    with pytest.raises(NotImplementedError, match="num_beams"):
        generation_plan(dict(num_beams=9))
    with pytest.raises(NotImplementedError, match="top_k"):
        generation_plan(dict(top_k=5))
    with pytest.raises(ValueError, match="num_return_sequences"):
        generation_plan(dict(num_beams=2, num_return_sequences=3))
    assert generation_plan({}) == dict(num_beams=1, num_return_sequences=1, length_penalty=1.0, early_stopping=False, eos_token_id=None)
    assert generation_plan(dict(num_beams=1, do_sample=False), decoder_input_ids=object())["num_beams"] == 1      # greedy keeps the prompt branch
    got = generation_plan(dict(num_beams=4, num_return_sequences=2, length_penalty=2, early_stopping="never", eos_token_id=[7]))
    assert got == dict(num_beams=4, num_return_sequences=2, length_penalty=2.0, early_stopping="never", eos_token_id=7)
