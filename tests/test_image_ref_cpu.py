"""CPU: tests/_image_ref.py - the numpy restatement of the reference's image_preprocessor that the plan tests and the GPU tests compare
with - IS PIL's arithmetic: equal to PIL / torch / HF bit for bit on every case, and to the committed fixture."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_ref as R  # noqa: E402

Image = pytest.importorskip("PIL.Image")

IDS = [R.case_name(*c) for c in R.CASES]


def pil_u8(img, n_px, rule):
    H, W, _ = img.shape
    oh, ow = R.output_size(H, W, n_px)
    top, left = R.crop_box(oh, ow, n_px, rule)
    im = Image.fromarray(img).resize((ow, oh), Image.BICUBIC)
    return np.array(im.crop((left, top, left + n_px, top + n_px)))


def test_the_cases_are_the_ones_the_spec_was_pinned_on():
    assert len(R.CASES) == 26 and (600, 450, 8) in R.SIZES
    # both rules are exercised where they differ: some case has an odd crop margin on an axis
    odd = [(H, W, n) for H, W, n in R.SIZES if R.crop_box(*R.output_size(H, W, n), n, "round") != R.crop_box(*R.output_size(H, W, n), n, "floor")]
    assert odd
    assert R.output_size(600, 450, 8) == (10, 8) and R.coeffs(450, 8)[0] == 227 and R.coeffs(600, 10)[0] == 241      # scales 56.25 and 60


@pytest.mark.parametrize("H,W,n_px,kind", R.CASES, ids=IDS)
@pytest.mark.parametrize("rule", ["round", "floor"])
def test_uint8_level_equals_pil_resize_and_crop(H, W, n_px, kind, rule):
    img = R.case_image(H, W, kind)
    got = R.resize_crop_u8(img, n_px, rule)
    assert got.dtype == np.uint8 and np.array_equal(got, pil_u8(img, n_px, rule))


def test_checkerboards_reach_both_clamps():
    """Bicubic overshoots on a 0/255 checkerboard: some case's raw sums leave [0, 255] on both sides, so both clamps decide bytes."""
    lo = hi = False
    for H, W, n_px in R.SIZES:
        img = R.case_image(H, W, "checker")
        ow = R.output_size(H, W, n_px)[1]
        _, cs = R.coeffs(W, ow)
        for xmin, k in cs:
            acc = (img[:, xmin:xmin + len(k), :].astype(np.int64) * np.array(k)[None, :, None]).sum(1) + (1 << 21)
            lo, hi = lo or bool((acc >> 22).min() < 0), hi or bool((acc >> 22).max() > 255)
    assert lo and hi


@pytest.mark.parametrize("H,W,n_px,kind", R.CASES, ids=IDS)
def test_float_level_equals_the_torch_ops_of_totensor_and_normalize(H, W, n_px, kind):
    img = R.case_image(H, W, kind)
    u8 = pil_u8(img, n_px, "round")
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor(R.CLIP_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.as_tensor(R.CLIP_STD, dtype=torch.float32).view(3, 1, 1)
    want = t.sub_(mean).div_(std).numpy()
    got = R.preprocess(img, n_px, "round")
    assert got.dtype == np.float32 and np.array_equal(got, want)


@pytest.fixture(scope="module")
def hf_processor():
    transformers = pytest.importorskip("transformers")
    cls = getattr(transformers, "CLIPImageProcessor")
    return lambda n_px: cls(do_resize=True, size={"shortest_edge": n_px}, resample=3, do_center_crop=True,
                            crop_size={"height": n_px, "width": n_px}, do_rescale=False, do_normalize=False, do_convert_rgb=False)


@pytest.mark.parametrize("H,W,n_px,kind", R.CASES, ids=IDS)
def test_floor_rule_equals_hf_clip_image_processor(hf_processor, H, W, n_px, kind):
    img = R.case_image(H, W, kind)
    out = hf_processor(n_px)(images=[img], return_tensors="np", input_data_format="channels_last")["pixel_values"][0]   # [3, n_px, n_px], unscaled
    want = np.asarray(out)
    got = R.resize_crop_u8(img, n_px, "floor").transpose(2, 0, 1)
    assert want.shape == got.shape and np.array_equal(want.astype(np.int64), got.astype(np.int64))


def test_the_committed_fixture_is_pil(golden):
    """tests/golden/clip_preprocess.npz (what the GPU tests compare with) holds PIL's results for exactly these inputs."""
    z = golden("clip_preprocess.npz")
    assert len(z) == 3 * len(R.CASES)
    for H, W, n_px, kind in R.CASES:
        name = R.case_name(H, W, n_px, kind)
        img = R.case_image(H, W, kind)
        assert bytes(z["sha/" + name]) == hashlib.sha256(img.tobytes()).digest()
        for rule in ("round", "floor"):
            assert z[f"{rule}/{name}"].dtype == np.float32
            assert np.array_equal(z[f"{rule}/{name}"], R.preprocess(img, n_px, rule))
            lut = R.normalize_table()
            u8 = pil_u8(img, n_px, rule)
            assert np.array_equal(z[f"{rule}/{name}"], np.stack([lut[c][u8[:, :, c]] for c in range(3)]))
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_preprocess.npz")) < 512 * 1024
