"""CPU: the plain-torch restatement of the CLIP text tower (tests/_clip_text_ref.py), which the GPU tests at real widths compare against,
equals HF ``CLIPTextModelWithProjection`` on the committed fixture (tests/golden/make_golden_clip_text.py)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _clip_text_ref import encode_text_ref  # noqa: E402
from conftest import load_golden  # noqa: E402


def test_restatement_matches_the_hf_fixture():
    z = load_golden("clip_text.npz")
    sd = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("w.")}
    ids = torch.from_numpy(z["ids"])
    got = encode_text_ref(sd, int(z["cfg"][2]), ids)
    want = torch.from_numpy(z["text_embeds"]).double()
    assert got.shape == want.shape == (7, 64)
    assert (got - want).abs().max().item() <= 1e-5
    # the fixture's own property: ids behind the EOT do not reach the pooled row
    assert torch.equal(ids[6, :13], ids[2, :13]) and not torch.equal(ids[6], ids[2])
    assert (want[6] - want[2]).abs().max().item() <= 1e-5


def test_configs_and_random_init_shapes():
    from eavqa_amd.models.clip_text import KNOWN_TEXT_TOWERS, TextConfig, random_init_text_state_dict
    assert {n: (c.width, c.n_head, c.n_layer, c.proj, c.context, c.vocab) for n, c in KNOWN_TEXT_TOWERS.items()} == {
        "ViT-B/32": (512, 8, 12, 512, 77, 49408), "ViT-B/16": (512, 8, 12, 512, 77, 49408),
        "ViT-L/14": (768, 12, 12, 768, 77, 49408), "ViT-L/14@336px": (768, 12, 12, 768, 77, 49408)}
    cfg = TextConfig(64, 2, 1, 256, 32, context=77, vocab=300)
    sd = random_init_text_state_dict(cfg, 3)
    assert sd["text_model.embeddings.token_embedding.weight"].shape == (300, 64)
    assert sd["text_model.embeddings.position_embedding.weight"].shape == (77, 64)
    assert sd["text_projection.weight"].shape == (32, 64)
    assert sd["text_model.encoder.layers.1.mlp.fc1.weight"].shape == (256, 64)
    again = random_init_text_state_dict(cfg, 3)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
