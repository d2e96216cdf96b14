"""Numpy restatement of the reference's ``image_preprocessor`` (OpenAI CLIP ``_transform``: ``Resize(n_px, BICUBIC)`` on an 8-bit PIL image,
``CenterCrop(n_px)``, ``ToTensor``, ``Normalize``; src/tools/extract_clip_embeddings_conceptual_captions.py:26,61), written tap by tap the
way PIL's 8-bit resampler computes it.  tests/test_image_ref_cpu.py pins it to PIL itself; the GPU tests and the plan tests compare the
product code with it, so they need neither PIL nor torchvision.  Also the shared test cases and their (seeded, fully specified) images.
"""
import math

import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22

# (H, W, n_px): up- and down-scaling, identity on one or both axes, windows clipped at both borders, inputs smaller than the filter
# support, odd crop margins (where "round" and "floor" differ), tall and wide extremes; the last one has 227 taps
SIZES = [(48, 64, 28), (64, 48, 28), (150, 200, 28), (20, 13, 28), (3, 5, 28), (28, 90, 28), (61, 28, 28), (28, 28, 28),
         (333, 37, 8), (5, 600, 8), (97, 131, 32), (33, 47, 32), (600, 450, 8)]
KINDS = ("random", "checker")
CASES = [(H, W, n, kind) for (H, W, n) in SIZES for kind in KINDS]


def case_name(H, W, n_px, kind):
    return f"{H}x{W}_to{n_px}_{kind}"


def case_image(H, W, kind, seed=2021):
    """uint8 [H, W, 3].  "checker": a 0/255 checkerboard (bicubic overshoots on it: both clamps), shifted by one per channel.
    "random": splitmix64 of the element index, written out here so that the bytes depend on no library's generator."""
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    if kind == "checker":
        return (((y + x + c) & 1) * 255).astype(np.uint8)
    z = ((y * W + x) * 3 + c).astype(np.uint64) + np.uint64(seed * 1000003 + H * 4099 + W)
    z = z * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(56)).astype(np.uint8)


def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """Per output index: (xmin, [int k ...]) - the window start and the 22-bit fixed-point weights of one axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [bicubic((x + xmin - center + 0.5) / fs) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS)) for v in w]
        assert len(k) <= ksize
        out.append((xmin, k))
    return ksize, out


def resample_axis(img, out_size, axis, lo=0, hi=None):
    """One 8-bit pass along ``axis`` (0 rows, 1 columns) for the output indices [lo, hi)."""
    hi = out_size if hi is None else hi
    _, cs = coeffs(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    res = np.empty((hi - lo,) + src.shape[1:], dtype=np.uint8)
    for o in range(lo, hi):
        xmin, k = cs[o]
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t, kv in enumerate(k):
            acc += src[xmin + t] * kv
        assert np.abs(acc).max() < 2 ** 31                       # int32 suffices
        res[o - lo] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(res, 0, axis)


def output_size(H, W, n_px):
    """torchvision ``Resize(int)``: the shorter side becomes n_px, the longer one int(n_px * long / short).  (oh, ow)"""
    if H <= W:
        return n_px, int(n_px * W / H)
    return int(n_px * H / W), n_px


def crop_box(oh, ow, n_px, crop_offset="round"):
    """(top, left): torchvision ``CenterCrop`` rounds half to even (Python ``round``), HF ``CLIPImageProcessor`` floors."""
    if crop_offset == "round":
        return int(round((oh - n_px) / 2.0)), int(round((ow - n_px) / 2.0))
    if crop_offset == "floor":
        return (oh - n_px) // 2, (ow - n_px) // 2
    raise ValueError(crop_offset)


def resize_crop_u8(img, n_px, crop_offset="round"):
    """uint8 [n_px, n_px, 3]: horizontal pass, then vertical pass over its uint8 result, cropped."""
    H, W, _ = img.shape
    oh, ow = output_size(H, W, n_px)
    top, left = crop_box(oh, ow, n_px, crop_offset)
    mid = resample_axis(img, ow, 1, left, left + n_px)
    return resample_axis(mid, oh, 0, top, top + n_px)


def normalize_table(mean=CLIP_MEAN, std=CLIP_STD):
    """float32 [3, 256]: ``ToTensor`` then ``Normalize`` with the torch CPU ops those two transforms run."""
    import torch
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(3, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(3, 1)
    return v.view(1, 256).repeat(3, 1).sub_(m).div_(s).numpy()


def preprocess(img, n_px, crop_offset="round", mean=CLIP_MEAN, std=CLIP_STD):
    """float32 [3, n_px, n_px]: what ``image_preprocessor(PIL image)`` returns."""
    u8 = resize_crop_u8(img, n_px, crop_offset)
    lut = normalize_table(mean, std)
    return np.stack([lut[c][u8[:, :, c]] for c in range(3)]).astype(np.float32)
