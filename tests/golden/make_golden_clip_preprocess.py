"""Writes tests/golden/clip_preprocess.npz: what the reference's ``image_preprocessor`` (OpenAI CLIP ``_transform``) returns for the cases
of tests/_image_ref.py, computed with PIL (``Image.resize(BICUBIC)``, ``Image.crop``) and the torch ops of ``ToTensor`` / ``Normalize`` -
none of the code under test.  The GPU box may have no PIL: the GPU tests read only this file and tests/_image_ref.py.

Per case ``<name>`` (``_image_ref.case_name``): ``round/<name>`` and ``floor/<name>`` float32 [3, n_px, n_px] for the two crop rules, and
``sha/<name>``, the SHA-256 of the input image's bytes.  The inputs themselves are ``_image_ref.case_image`` (a written-out integer hash, so
they are the same bytes everywhere); the 600x450 one alone would be most of the size limit of a committed file.

    python tests/golden/make_golden_clip_preprocess.py
"""
import hashlib
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _image_ref as R  # noqa: E402


def pil_u8(img, n_px, rule):
    H, W, _ = img.shape
    oh, ow = R.output_size(H, W, n_px)
    top, left = R.crop_box(oh, ow, n_px, rule)
    im = Image.fromarray(img).resize((ow, oh), Image.BICUBIC)
    return np.array(im.crop((left, top, left + n_px, top + n_px)))


def to_tensor_normalize(u8):
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)    # ToTensor
    mean = torch.as_tensor(R.CLIP_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.as_tensor(R.CLIP_STD, dtype=torch.float32).view(3, 1, 1)
    return t.sub_(mean).div_(std).numpy()                                                                      # Normalize


def main():
    out = {}
    for H, W, n_px, kind in R.CASES:
        name = R.case_name(H, W, n_px, kind)
        img = R.case_image(H, W, kind)
        out["sha/" + name] = np.frombuffer(hashlib.sha256(img.tobytes()).digest(), dtype=np.uint8)
        for rule in ("round", "floor"):
            out[f"{rule}/{name}"] = to_tensor_normalize(pil_u8(img, n_px, rule))
    path = os.path.join(HERE, "clip_preprocess.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
