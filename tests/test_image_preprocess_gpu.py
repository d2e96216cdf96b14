"""GPU: CLIP image preprocessing on the card (csrc/image.hip behind eavqa_amd.models.clip_preprocess) - raw uint8 images to what the
reference's image_preprocessor returns, BIT FOR BIT.  The expected values are PIL's (tests/golden/clip_preprocess.npz, written by
tests/golden/make_golden_clip_preprocess.py; tests/test_image_ref_cpu.py ties the fixture, PIL and tests/_image_ref.py together), so this
file needs neither PIL nor torchvision."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_ref as R  # noqa: E402
from conftest import load_golden  # noqa: E402

DEV = "cuda"
IDS = [R.case_name(*c) for c in R.CASES]
RULES = ["round", "floor"]


@pytest.fixture(scope="module")
def fixture():
    """name -> (image, {rule: expected float32 [3, n, n] tensor}); computed once, never modified."""
    z = load_golden("clip_preprocess.npz")
    out = {}
    for H, W, n_px, kind in R.CASES:
        name = R.case_name(H, W, n_px, kind)
        img = R.case_image(H, W, kind)
        assert bytes(z["sha/" + name]) == hashlib.sha256(img.tobytes()).digest(), name
        out[name] = (img, {r: torch.from_numpy(z[f"{r}/{name}"]) for r in RULES})
    return out


@pytest.fixture(scope="module")
def P():
    from eavqa_amd.models import clip_preprocess
    return clip_preprocess


def names_of(n_px):
    return [R.case_name(*c) for c in R.CASES if c[2] == n_px]


# ------------------------------------------------------------------ form (a): float32 NCHW

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("H,W,n_px,kind", R.CASES, ids=IDS)
def test_single_image_equals_pil(P, fixture, H, W, n_px, kind, rule):
    img, want = fixture[R.case_name(H, W, n_px, kind)]
    got = P.ClipImagePreprocessor(n_px, crop_offset=rule, device=DEV)([img])
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, n_px, n_px) and got.is_cuda
    assert torch.equal(got[0].cpu(), want[rule])


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("n_px", [28, 8, 32])
def test_ragged_batch_equals_pil(P, fixture, n_px, rule):
    """Every case of one n_px in ONE call: 16 / 6 / 4 images of different sizes behind one descriptor table and one tile grid."""
    names = names_of(n_px)
    pre = P.ClipImagePreprocessor(n_px, crop_offset=rule, device=DEV)
    batch = P.ImageBatch([fixture[n][0] for n in names])
    got = pre(batch).cpu()
    assert tuple(got.shape) == (len(names), 3, n_px, n_px)
    for i, n in enumerate(names):
        assert torch.equal(got[i], fixture[n][1][rule]), n
    assert torch.equal(pre(batch).cpu(), got)                                # the cached plan and device tables: the same again


def test_other_mean_and_std_go_through_the_table(P, fixture):
    img, _ = fixture[R.case_name(97, 131, 32, "random")]
    mean, std = (0.5, 0.25, 0.125), (0.5, 2.0, 0.3)
    got = P.ClipImagePreprocessor(32, mean=mean, std=std, device=DEV)([img])[0].cpu()
    assert np.array_equal(got.numpy(), R.preprocess(img, 32, "round", mean, std))


# ------------------------------------------------------------------ form (b): eavqa_patchify's patch rows

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_px,ps,ldp", [(28, 14, 608), (32, 16, 768)], ids=["p14-pad", "p16-nopad"])
def test_patch_rows_equal_patchify_of_the_pixels(P, fixture, n_px, ps, ldp, dtype, rule):
    """K = 588 -> ldp 608 (pad columns must be WRITTEN as zero: the output starts as NaN) and K = 768 = ldp."""
    from eavqa_amd import ops
    names = names_of(n_px)
    pre = P.ClipImagePreprocessor(n_px, crop_offset=rule, device=DEV)
    batch = P.ImageBatch([fixture[n][0] for n in names])
    pixels = pre(batch)
    want = ops.patchify(pixels, ps, dtype, ldp)
    g = n_px // ps
    out = torch.full((len(names) * g * g, ldp), float("nan"), device=DEV, dtype=dtype)
    got = pre.patches(batch, ps, dtype, ldp, out=out)
    assert got is out and got.dtype == dtype
    assert not torch.isnan(got).any()
    assert torch.equal(got.view(torch.int32 if dtype == torch.float32 else torch.int16), want.view(torch.int32 if dtype == torch.float32 else torch.int16))
    assert (got[:, 3 * ps * ps:] == 0).all()
    # and the pixels inside the rows are PIL's
    first = got[:g * g, :3 * ps * ps].float().cpu().view(g, g, 3, ps, ps).permute(2, 0, 3, 1, 4).reshape(3, n_px, n_px)
    exp = fixture[names[0]][1][rule]
    assert torch.equal(first, exp if dtype == torch.float32 else exp.to(torch.bfloat16).float())


# ------------------------------------------------------------------ interfaces

@pytest.fixture(scope="module")
def tiny_vit():
    from eavqa_amd.models.clip_vit import ClipVisionEncoder, ViTConfig, random_init_vit_state_dict
    vcfg = ViTConfig(64, 2, 2, 128, 14, 28, 24)                    # width, layers, heads, mlp, patch, image, projection: K = 588 -> 608
    return ClipVisionEncoder(vcfg, random_init_vit_state_dict(vcfg, 5, DEV), torch.bfloat16, DEV)


def test_encode_raw_equals_encode_image_of_the_preprocessed_pixels(P, fixture, tiny_vit):
    images = [fixture[n][0] for n in names_of(28)]
    pre = P.ClipImagePreprocessor(28, device=DEV)
    want = tiny_vit.encode_image(pre(images))
    got = tiny_vit.encode_raw(images)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(images), 24)
    assert torch.equal(got, want)
    assert torch.equal(tiny_vit.encode_raw(P.ImageBatch(images)), want)
    floor = P.ClipImagePreprocessor(28, crop_offset="floor", device=DEV)
    got_floor = tiny_vit.encode_raw(images, preprocessor=floor)
    assert torch.equal(got_floor, tiny_vit.encode_image(floor(images))) and not torch.equal(got_floor, want)
    with pytest.raises(ValueError):
        tiny_vit.encode_raw(images, preprocessor=P.ClipImagePreprocessor(32, device=DEV))


def test_encode_ahead_takes_an_image_batch(P, fixture, tiny_vit):
    from eavqa_amd.models.clip_vit import EncodeAhead
    names = names_of(28)
    groups = [names[:5], names[5:11], names[11:]]
    batches = [P.ImageBatch([fixture[n][0] for n in grp]) for grp in groups]
    want = [tiny_vit.encode_raw(b) for b in batches]
    ahead = EncodeAhead(tiny_vit)
    ticket = ahead.submit(batches[0])
    for i in range(len(batches)):
        emb = ahead.result(ticket)
        if i + 1 < len(batches):
            ticket = ahead.submit(batches[i + 1])
        torch.cuda.synchronize()
        assert torch.equal(emb, want[i]), i


def test_executor_images_route_equals_its_pixel_values_route(P, fixture, tiny_vit):
    from eavqa_amd.trainers.clipcap_executor import ClipCapExecutor
    ex = ClipCapExecutor(None, None, vision_encoder=tiny_vit, model=object(), device=DEV)
    images = [fixture[n][0] for n in names_of(28)][:6]
    pixels = P.ClipImagePreprocessor(28, device=DEV)(images)
    want = ex._clip_embeddings({"pixel_values": pixels})
    assert torch.equal(ex._clip_embeddings({"images": images}), want)
    assert torch.equal(ex._clip_embeddings({"images": P.ImageBatch(images)}), want)
    rows = [images[0:2], images[2:4], images[4:6]]                           # several images per row -> [B, n, D]
    want3 = ex._clip_embeddings({"pixel_values": pixels.view(3, 2, 3, 28, 28)})
    got3 = ex._clip_embeddings({"images": rows})
    assert tuple(got3.shape) == (3, 2, 24) and torch.equal(got3, want3)
    with pytest.raises(ValueError):
        ex._clip_embeddings({"images": [images[0:2], images[2:3]]})
    emb = torch.randn(4, 24)
    assert torch.equal(ex._clip_embeddings({"clip_embeddings": emb, "images": images}).cpu(), emb)       # as today: stored embeddings win


# ------------------------------------------------------------------ the C ABI rejects before any launch

def _call(lib, name, **over):
    """One of the two entry points on a small valid problem (16 stands for an aligned device pointer, 18 for a misaligned one) with the
    named arguments replaced.  Only ever called WITH a fault: a valid call would go on to enqueue a kernel on these pointers."""
    a = dict(dtype=0, n_px=28, ps=14, n_images=2, n_tiles=4, src=16, src_bytes=4096, desc=16, tables=16, n_table_words=1024, tiles=16,
             mid=16, mid_bytes=4096, mid_stride=84, lut=16, out=16, ldp=608, stream=None)
    assert over and not set(over) - set(a), over
    a.update(over)
    order = {
        "rows": ("n_px", "n_images", "n_tiles", "src", "src_bytes", "desc", "tables", "n_table_words", "tiles", "mid", "mid_bytes", "mid_stride",
                 "stream"),
        "emit": ("dtype", "n_px", "ps", "n_images", "desc", "tables", "n_table_words", "mid", "mid_bytes", "mid_stride", "lut", "out", "ldp",
                 "stream"),
    }
    return getattr(lib, "eavqa_clip_resize_" + name)(*[a[n] for n in order[name]])


# (entry point, the fault, code): -1 ARG, -2 ALIGN, -3 SHAPE, -4 DTYPE
REJECTIONS = [
    ("rows", dict(src=None), -1), ("rows", dict(desc=None), -1), ("rows", dict(tables=None), -1), ("rows", dict(tiles=None), -1),
    ("rows", dict(mid=None), -1), ("rows", dict(n_px=0), -1), ("rows", dict(n_images=0), -1), ("rows", dict(n_tiles=0), -1),
    ("rows", dict(src_bytes=0), -1), ("rows", dict(mid_bytes=0), -1), ("rows", dict(n_table_words=0), -1),
    ("rows", dict(mid=18), -2), ("rows", dict(mid_stride=86), -2), ("rows", dict(mid_stride=80), -1), ("rows", dict(n_px=4100, mid_stride=12300), -3),
    ("emit", dict(desc=None), -1), ("emit", dict(tables=None), -1), ("emit", dict(mid=None), -1), ("emit", dict(lut=None), -1),
    ("emit", dict(out=None), -1), ("emit", dict(n_px=-28), -1), ("emit", dict(n_images=0), -1), ("emit", dict(ps=-1), -1),
    ("emit", dict(ps=16), -3),                                  # n_px = 28 is no multiple of the patch size
    ("emit", dict(ps=3), -3),
    ("emit", dict(dtype=7), -4), ("emit", dict(dtype=2), -4),   # an unknown dtype; half is no patch-row type
    ("emit", dict(dtype=1, ps=0), -4),                          # NCHW pixels are float32
    ("emit", dict(dtype=7, ps=0), -4),
    ("emit", dict(ldp=587), -1), ("emit", dict(dtype=1, ldp=0), -1),         # ldp below 3 * ps * ps = 588
    ("emit", dict(mid=18), -2), ("emit", dict(mid_stride=86), -2), ("emit", dict(mid_stride=80), -1),
    ("emit", dict(dtype=7, out=None), -1),                      # null pointers before the dtype, the dtype before the shape
    ("emit", dict(dtype=7, ps=16), -4),
    ("emit", dict(ps=16, ldp=0), -3),
]


@pytest.mark.parametrize("name,fault,code", REJECTIONS, ids=[f"{n}-{'-'.join(f'{k}_{v}' for k, v in f.items())}" for n, f, _ in REJECTIONS])
def test_abi_rejections_happen_before_any_launch(name, fault, code):
    from eavqa_amd import _lib
    lib = _lib.load()
    before = torch.cuda.memory_allocated()
    assert _call(lib, name, **fault) == code
    torch.cuda.synchronize()                                                 # nothing was enqueued on these stand-in pointers: no fault surfaces
    assert torch.cuda.memory_allocated() == before                           # and nothing was allocated
