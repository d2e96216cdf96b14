"""CPU: training on interleaved image-text rows - the reference of the GPU tests (tests/_incontext_ref.py) against the oracle's
``insert_prefix_into_input`` and against tests/golden/incontext.npz (the reference's code + HF), and the host plan
``models/interleave.py``, which imports without a GPU."""
import numpy as np
import pytest
import torch

import _incontext_ref as ref
from conftest import load_golden

ATOL = 2e-5                         # tests/test_oracle_golden.py, the tiny GPT-2 / OPT
# the tiny T0: the bounds of tests/test_oracle_t5.py (test_oracle_golden.py holds no T5 model): loss and logits absolute, the gradient
# relative to max(1, max |want|).  As there, the oracle runs in float32, the precision of the fixture's producer.
T5_TOL = dict(logits=2e-5, loss=1e-5, grad=1e-5)


def _rows(seed, B, T, n_img, special):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(3, special - n_img - 1, (B, T), generator=g)
    for b in range(B):
        for i, p in enumerate(sorted(torch.randperm(T, generator=g)[:n_img].tolist())):
            tok[b, p] = special - i
    labels = torch.randint(3, special - n_img - 1, (B, T), generator=g)
    labels[torch.rand(B, T, generator=g) < 0.5] = -100
    return tok, labels


@pytest.mark.parametrize("L,n_img", [(1, 1), (1, 3), (3, 1), (3, 3), (10, 5)])
def test_label_layout_is_insert_prefix_on_the_labels(L, n_img):
    special = 90
    tok, labels = _rows(L * 10 + n_img, 4, 70, n_img, special)
    labels[0, (tok[0] == special).nonzero()[0, 0]] = 7                 # a label ON a sentinel is dropped
    got, scored = ref.expand_labels(tok, labels, L, n_img, special)
    want = ref.expand_labels_by_oracle(tok, labels, L, n_img, special)
    assert np.array_equal(got, want)
    assert scored.tolist() == (want != -100).sum(1).tolist()
    assert got.shape == (4, 70 + (L - 1) * n_img)


def test_label_layout_with_too_few_and_too_many_sentinels():
    special, L, n_img = 50, 3, 2
    tok = np.array([[5, 50, 6, 7, 8, 9], [50, 49, 48 + 2, 6, 7, 8]])     # row 0: one sentinel of two; row 1: three sentinels
    labels = np.array([[1, 2, 3, -100, 4, 5], [1, 2, 3, 4, 5, 6]])
    out, scored = ref.expand_labels(tok, labels, L, n_img, special)
    assert out.shape == (2, 10)
    assert out[0].tolist() == [1, -100, -100, -100, 3, -100, 4, 5, -100, -100] and scored[0] == 4      # a defined -100 tail
    assert out[1].tolist() == [-100] * 9 + [4] and scored[1] == 1        # text pushed out of the row by the surplus sentinel is dropped


@pytest.mark.parametrize("arch", ["gpt2", "opt"])
def test_causal_oracle_composition_matches_fixture(arch):
    f = load_golden("incontext.npz")
    sd, cfg, mapper, mcfg = ref.causal_pieces(load_golden(f"clipcap_{arch}_mlp.npz"), arch)
    assert int(f[f"{arch}.L"]) == mcfg["prefix_length"]
    for name, tok, mask, prefix, labels, special in ref.fixture_cases(f, arch):
        loss, logits, grads, full = ref.causal_oracle(sd, cfg, mapper, mcfg, tok, prefix, mask, labels, 3, special, dtype=torch.float32)
        assert np.array_equal(full.numpy(), f[f"{arch}.{name}.labels_out"])
        assert torch.allclose(logits.float(), torch.from_numpy(f[f"{arch}.logits"]), atol=ATOL), name
        assert abs(float(loss) - float(f[f"{arch}.{name}.loss"])) < ATOL, name
        for k, g in grads.items():
            assert torch.allclose(g.float(), torch.from_numpy(f[f"{arch}.{name}.gmap.{k}"]), atol=ATOL), (name, k)
            assert g.abs().max() > 0 and torch.isfinite(g).all()


def test_t5_oracle_composition_matches_fixture():
    f = load_golden("incontext.npz")
    sd, cfg, mapper, mcfg = ref.t5_pieces(load_golden("vct0_t0.npz"))
    for name, tok, mask, prefix, labels, special in ref.fixture_cases(f, "t0"):
        loss, logits, grads = ref.t5_oracle(sd, cfg, mapper, mcfg, tok, prefix, mask, labels, 3, special, dtype=torch.float32)
        assert (logits - torch.from_numpy(f[f"t0.{name}.logits"])).abs().max().item() <= T5_TOL["logits"], name
        assert abs(float(loss) - float(f[f"t0.{name}.loss"])) <= T5_TOL["loss"], name
        for k, g in grads.items():
            want = torch.from_numpy(f[f"t0.{name}.gmap.{k}"])
            assert (g.float() - want).abs().max().item() <= T5_TOL["grad"] * max(1.0, want.abs().max().item()), (name, k)
            assert g.abs().max() > 0 and torch.isfinite(g).all()


def test_fixture_inputs_are_the_shared_episode():
    f = load_golden("incontext.npz")
    for arch in ("gpt2", "opt"):
        V = int(load_golden(f"clipcap_{arch}_mlp.npz")["cfg"][0])
        tok, mask, last, every = ref.episode(V, V - 5)
        for k, want in (("tokens", tok), ("mask", mask), ("last.labels", last), ("all.labels", every)):
            assert np.array_equal(f[f"{arch}.{k}"], want.numpy()), (arch, k)
        sent = ref.is_sentinel(tok.numpy(), 3, V - 5)
        assert (sent.sum(1) == 3).all() and sent.argmax(1).tolist() == [0, 1, 0]      # positions differ between rows
        assert mask[1, -2:].sum() == 0 and mask.sum() == mask.numel() - 2


# ------------------------------------------------------------------------------------------------ interleave_plan
def test_interleave_plan_lengths_and_counts():
    from eavqa_amd.models.interleave import interleave_plan
    V = 96
    tok, mask, last, every = ref.episode(V, V - 5)
    for labels in (last, every, None):
        for L in (1, 3, 10):
            p = interleave_plan(tok, mask, labels, L, 3, V - 5)
            lengths, count, T_out = ref.plan(tok.numpy(), mask.numpy(), None if labels is None else labels.numpy(), L, 3, V - 5)
            assert (p.lengths, p.label_count, p.T_out) == (lengths, count, T_out)
    # no mask: every position is attended; a label on a sentinel is not counted
    lab = last.clone()
    lab[0, 0] = 5                                                  # row 0 holds a sentinel at position 0
    p = interleave_plan(tok, None, lab, 3, 3, V - 5)
    assert p.lengths == [tok.shape[1] + 2 * 3] * 3 and p.label_count == int((last != -100).sum())
    assert p.label_count == int(ref.expand_labels(tok.numpy(), lab.numpy(), 3, 3, V - 5)[1].sum())


def test_interleave_plan_counts_a_sentinel_under_a_zero_mask():
    from eavqa_amd.models.interleave import interleave_plan
    tok = torch.tensor([[90, 4, 5, 89, 6, 7]])
    mask = torch.tensor([[0, 1, 1, 1, 1, 0]])                      # the first sentinel sits under a zero mask: still an image
    p = interleave_plan(tok, mask, None, 4, 2, 90)
    assert p.lengths == [3 + 4 * 2] and p.T_out == 6 + 3 * 2 and p.label_count is None


@pytest.mark.parametrize("row", [[4, 5, 90, 6, 7, 8], [90, 89, 90, 6, 7, 8], [4, 5, 6, 7, 8, 9]], ids=["too_few", "too_many", "none"])
def test_interleave_plan_rejects_a_wrong_sentinel_count(row):
    from eavqa_amd.models.interleave import interleave_plan
    tok = torch.tensor([[90, 4, 89, 5, 6, 7], row])                # two images per row: ids 90 and 89; row 0 is well formed
    with pytest.raises(ValueError, match="every row must hold exactly one sentinel token per image"):
        interleave_plan(tok, torch.ones_like(tok), None, 3, 2, 90)


def test_interleave_plan_checks_shapes():
    from eavqa_amd.models.interleave import interleave_plan
    tok = torch.tensor([[90, 4, 5]])
    with pytest.raises(ValueError, match="labels"):
        interleave_plan(tok, None, torch.zeros(1, 4, dtype=torch.long), 2, 1, 90)
    with pytest.raises(ValueError, match="question_mask"):
        interleave_plan(tok, torch.ones(2, 3, dtype=torch.long), None, 2, 1, 90)
