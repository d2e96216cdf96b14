"""GPU: the CLIP text tower (models/clip_text.py) - the HF fixture, the row-plan kernel against numpy, real widths against the plain-torch
restatement (tests/_clip_text_ref.py, itself pinned to the fixture by tests/test_clip_text_ref_cpu.py) and the chunking of large batches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _clip_text_ref import encode_text_ref  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOS, EOT = 49406, 49407
FP32_TOL, BF16_TOL = 2e-4, 5e-2          # the bounds of the vision tower's fixture test (test_model_gpu.py)


def make_ids(lengths, seed, vocab=49408, context=77):
    """clip.tokenize-shaped rows: <BOS> tokens <EOT> 0 ...; ``lengths`` count BOS and EOT (2 = the empty string)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros((len(lengths), context), dtype=torch.int64)
    for r, n in enumerate(lengths):
        ids[r, 0] = vocab - 2
        ids[r, 1:n - 1] = torch.randint(1, vocab - 2, (n - 2,), generator=g)
        ids[r, n - 1] = vocab - 1
    return ids


def encoder(cfg, sd, dtype, pack):
    from eavqa_amd.models.clip_text import ClipTextEncoder
    return ClipTextEncoder(cfg, sd, dtype, DEV, pack=pack)


@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_clip_text_matches_hf_fixture(dtype, pack):
    from eavqa_amd.models.clip_text import TextConfig
    z = load_golden("clip_text.npz")
    V, W, NH, NL, MLP, P, CTX = [int(v) for v in z["cfg"]]
    sd = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("w.")}
    enc = encoder(TextConfig(W, NL, NH, MLP, P, context=CTX, vocab=V), sd, dtype, pack)
    ids = torch.from_numpy(z["ids"])
    emb = enc.encode_text(ids)
    assert emb.dtype == torch.float32 and emb.shape == (ids.shape[0], P) and emb.is_cuda
    err = (emb.cpu() - torch.from_numpy(z["text_embeds"])).abs().max().item()
    print(f"clip_text fixture {dtype} pack={pack}: max |d text_embeds| = {err:.3e}")
    assert err <= (FP32_TOL if dtype == torch.float32 else BF16_TOL), err
    assert torch.equal(enc.encode_text(ids.to(DEV)), emb)            # ids on the device: the same rows
    if pack:                                                         # ids behind the EOT never enter a packed batch
        assert torch.equal(emb[6], emb[2])


@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("pack", [True, False])
def test_clip_text_plan_exact(B, pack):
    from eavqa_amd import ops
    special = [2, 64, 65, 77]
    cases = [[n] for n in special] if B == 1 else [None]
    for only in cases:
        if only is None:
            lengths = torch.randint(2, 78, (B,), generator=torch.Generator().manual_seed(B)).tolist()
            for i, n in enumerate(special):
                lengths[i * (B - 1) // 3] = n
        else:
            lengths = only
        ids = make_ids(lengths, 100 + B)
        if B == 7:
            ids[3, 40:] = torch.randint(1, EOT, (37,), generator=torch.Generator().manual_seed(1))     # ids behind the EOT
            ids[3, lengths[3] - 1] = EOT
        a = ids.numpy()
        eot = a.argmax(axis=1)
        lens = eot + 1 if pack else np.full(B, 77)
        cu = np.concatenate([[0], np.cumsum(lens)])
        got = [t.cpu().numpy() for t in ops.clip_text_plan(ids.to(DEV), pack)]
        M = int(cu[-1])
        assert np.array_equal(got[0], eot) and got[0].dtype == np.int32
        assert np.array_equal(got[1], cu)
        assert np.array_equal(got[2][:M], np.concatenate([a[b, :lens[b]] for b in range(B)]))
        assert np.array_equal(got[3][:M], np.concatenate([np.arange(lens[b]) for b in range(B)]))
        assert np.array_equal(got[4], cu[:-1] + eot)
        if only is None and pack:
            assert [int(n) for n in lens[[lengths.index(s) for s in special]]] == special


REAL_LENGTHS = [2, 64, 65, 77, 9, 12, 31, 70]


@pytest.fixture(scope="module", params=["ViT-L/14", "ViT-B/32"])
def real_tower(request):
    """(cfg, weights, ids, float64 reference): the tower at its real width, cut to 2 layers, random init"""
    import dataclasses
    from eavqa_amd.models.clip_text import KNOWN_TEXT_TOWERS, random_init_text_state_dict
    cfg = dataclasses.replace(KNOWN_TEXT_TOWERS[request.param], n_layer=2)
    sd = random_init_text_state_dict(cfg, 2021)
    ids = make_ids(REAL_LENGTHS, 5)
    return cfg, sd, ids, encode_text_ref(sd, cfg.n_head, ids)


@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_clip_text_real_widths(real_tower, dtype, pack):
    """Bounds: fp32 2e-4; bf16 5e-2 and a cosine >= 0.999 per row.  Measured on MI355X at this depth, packed = unpacked: fp32 max |d| 5.5e-6
    (width 768) / 3.5e-6 (512); bf16 max |d| 2.4e-2 / 2.3e-2 on values up to 4.3, min cosine 0.99997 - the bounds hold with room."""
    cfg, sd, ids, want = real_tower
    emb = encoder(cfg, sd, dtype, pack).encode_text(ids).cpu().double()
    err = (emb - want).abs().max().item()
    cos = torch.nn.functional.cosine_similarity(emb, want, dim=1).min().item()
    print(f"clip_text width {cfg.width} {dtype} pack={pack}: max |d| = {err:.3e}, min cosine = {cos:.6f}, max |ref| = {want.abs().max().item():.2f}")
    if dtype == torch.float32:
        assert err <= FP32_TOL, err
    else:
        assert err <= BF16_TOL, err
        assert cos >= 0.999, cos


def test_clip_text_chunks_large_batches():
    """B * H > 65 535: encode_text cuts the batch itself, and a row's embedding does not depend on its chunk."""
    from eavqa_amd.models.clip_text import ClipTextEncoder, TextConfig, random_init_text_state_dict
    cfg = TextConfig(128, 1, 2, 512, 128, vocab=512)
    enc = ClipTextEncoder(cfg, random_init_text_state_dict(cfg, 9), torch.float32, DEV)
    B = 40000
    assert B * cfg.n_head > 65535
    g = torch.Generator().manual_seed(4)
    lens = torch.randint(3, 7, (B,), generator=g)
    ids = torch.randint(1, 510, (B, 77), generator=g)
    pos = torch.arange(77)[None]
    ids = torch.where(pos < lens[:, None] - 1, ids, torch.zeros_like(ids))
    ids[:, 0] = 510
    ids[torch.arange(B), lens - 1] = 511
    emb = enc.encode_text(ids)
    assert emb.shape == (B, 128) and bool(torch.isfinite(emb).all())
    for r in (0, 32767, 32768, 39999):
        assert torch.equal(enc.encode_text(ids[r:r + 1])[0], emb[r]), r
