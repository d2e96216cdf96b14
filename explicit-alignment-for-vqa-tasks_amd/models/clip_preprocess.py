"""CLIP image preprocessing on the GPU: raw uint8 RGB images -> what the reference's ``image_preprocessor`` returns.

The reference's tower call is ``model.encode_image(image_preprocessor(img))`` (src/tools/extract_clip_embeddings_conceptual_captions.py:
26,61,69-73,83-88) with OpenAI CLIP's ``_transform``: ``Resize(n_px, BICUBIC)`` on an 8-bit PIL image, ``CenterCrop(n_px)``, ``ToTensor``,
``Normalize(mean, std)``.  PIL's 8-bit resampler is integer arithmetic (22-bit fixed-point weights, int32 sums, a horizontal pass and a
vertical pass over its uint8 result), so the GPU result is the same bit for bit.  This module is the host side: the packed batch, the
plan (coefficient tables, crop boxes, descriptors, tiles - numpy only, testable without a GPU) and the public ``ClipImagePreprocessor``;
the two kernels are csrc/image.hip.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22           # PIL: 32 - 8 - 2
H_TILE_ROWS = 16              # rows of the horizontal pass per workgroup (csrc/image.hip: IMG_H_TILE)
V_TILE_ROWS = 4               # output rows of the vertical pass per workgroup (IMG_V_TILE)
DESC_WORDS = 8                # int64 per image: src_off, W, H, row0, nrows, mid_off, table_x, table_y


class ImageBatch:
    """A list of uint8 ``[H, W, 3]`` arrays (or PIL RGB images, through ``np.asarray``), each with its own size, packed into ONE contiguous
    byte buffer - pinned when a GPU is present, so the whole batch goes to the card in one host -> device copy.  Mode conversion and
    decoding stay with the caller."""

    def __init__(self, images: Sequence):
        if isinstance(images, (np.ndarray, torch.Tensor)) or not len(images):
            raise TypeError("ImageBatch takes a non-empty list of uint8 [H, W, 3] images")
        arrays = []
        for i, im in enumerate(images):
            a = im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.dtype != np.uint8:
                raise TypeError(f"image {i}: dtype {a.dtype}, expected uint8 (decode and convert on the host)")
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"image {i}: shape {a.shape}, expected [H, W, 3] (RGB)")
            if a.shape[0] == 0 or a.shape[1] == 0:
                raise ValueError(f"image {i}: empty image {a.shape}")
            arrays.append(a)
        self.sizes: List[Tuple[int, int]] = [(int(a.shape[0]), int(a.shape[1])) for a in arrays]
        nbytes = np.array([h * w * 3 for h, w in self.sizes], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
        self.nbytes = int(nbytes.sum())
        self.data = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        flat = self.data.numpy()
        for a, o, n in zip(arrays, self.offsets, nbytes):
            flat[o:o + n] = a.reshape(-1)

    def __len__(self) -> int:
        return len(self.sizes)

    def image(self, i: int) -> np.ndarray:
        h, w = self.sizes[i]
        o = int(self.offsets[i])
        return self.data.numpy()[o:o + h * w * 3].reshape(h, w, 3)


def as_batch(images) -> ImageBatch:
    return images if isinstance(images, ImageBatch) else ImageBatch(images)


def output_size(H: int, W: int, n_px: int) -> Tuple[int, int]:
    """torchvision ``Resize(int)``: (oh, ow) with the shorter side n_px and the longer one int(n_px * long / short)."""
    if H <= W:
        return n_px, int(n_px * W / H)
    return int(n_px * H / W), n_px


def crop_offset_of(out: int, n_px: int, rule: str) -> int:
    if rule == "round":                                   # torchvision CenterCrop: Python round (half to even)
        return int(round((out - n_px) / 2.0))
    if rule == "floor":                                   # HF CLIPImageProcessor.center_crop
        return (out - n_px) // 2
    raise ValueError(f"crop_offset must be 'round' or 'floor', got {rule!r}")


def _bicubic(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def axis_table(in_size: int, out_size: int, lo: int, n: int) -> Tuple[int, np.ndarray, np.ndarray, np.ndarray]:
    """PIL's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the output indices [lo, lo + n) of one axis:
    (ksize, xmin int32 [n], count int32 [n], k int32 [n, ksize] zero past count).  ksize = ceil(support) * 2 + 1 grows with the
    scale (a 4000-pixel side to 224: 73 taps); nothing bounds it."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(lo, lo + n, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # astype truncates towards zero, as the C cast
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    t = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic((t + xmin[:, None] - center[:, None] + 0.5) / fs)
    w = np.where(t < count[:, None], w, 0.0)
    ww = np.zeros(n, dtype=np.float64)
    for j in range(ksize):                                                   # summed in tap order, as the C loop (a masked 0.0 adds nothing)
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    return ksize, xmin.astype(np.int32), count.astype(np.int32), k.astype(np.int32)


class PreprocessPlan:
    """Everything the two kernels need for one size signature ``(sizes, n_px, crop_offset)``, as flat host arrays:

    ``tables`` int32: one block per distinct (in, out) pair per axis - ``[ksize, xmin[n_px], count[n_px], k[n_px * ksize]]`` for the
        CROPPED output range only; ``table_offset[(axis, in, out)]`` is a block's word offset (images of one size share blocks);
    ``desc`` int64 [B, 8]: src_off, W, H, row0, nrows, mid_off, table_x, table_y - the horizontal pass runs over the input rows
        [row0, row0 + nrows) only, exactly those the vertical windows of the crop read, into ``mid`` (uint8, row stride ``mid_stride``);
    ``h_tiles`` int32 [n, 2]: (image, first row of the tile relative to row0): one grid over the ragged batch."""

    def __init__(self, sizes: Sequence[Tuple[int, int]], offsets: np.ndarray, n_px: int, crop_offset: str):
        self.n_px, self.crop_offset, self.B = n_px, crop_offset, len(sizes)
        self.mid_stride = (3 * n_px + 3) // 4 * 4                            # the vertical pass reads the rows four bytes at a time
        self.table_offset: Dict[Tuple[int, int, int], int] = {}
        self.boxes = []                                                      # (oh, ow, top, left) per image
        blocks, words, span = [], 0, {}
        desc = np.zeros((self.B, DESC_WORDS), dtype=np.int64)
        tiles = []
        mid_off = 0
        for i, (H, W) in enumerate(sizes):
            oh, ow = output_size(H, W, n_px)
            top, left = crop_offset_of(oh, n_px, crop_offset), crop_offset_of(ow, n_px, crop_offset)
            self.boxes.append((oh, ow, top, left))
            offs = []
            for axis, size, out, lo in ((1, W, ow, left), (0, H, oh, top)):
                key = (axis, size, out)
                if key not in self.table_offset:
                    ks, xmin, count, k = axis_table(size, out, lo, n_px)
                    self.table_offset[key] = words
                    span[key] = (int(xmin.min()), int((xmin + count).max()))
                    blocks += [np.array([ks], dtype=np.int32), xmin, count, k.reshape(-1)]
                    words += 1 + 2 * n_px + n_px * ks
                offs.append(self.table_offset[key])
            row0, row1 = span[(0, H, oh)]                                    # the input rows the vertical windows of the crop read
            desc[i] = (int(offsets[i]), W, H, row0, row1 - row0, mid_off, offs[0], offs[1])
            tiles += [(i, r) for r in range(0, row1 - row0, H_TILE_ROWS)]
            mid_off += (row1 - row0) * self.mid_stride
        self.tables = np.concatenate(blocks)
        self.desc, self.mid_bytes = desc, mid_off
        self.h_tiles = np.array(tiles, dtype=np.int32).reshape(-1, 2)
        self.src_bytes = int(offsets[-1]) + sizes[-1][0] * sizes[-1][1] * 3
        self._device: Dict[torch.device, Tuple[torch.Tensor, ...]] = {}

    def table(self, off: int):
        """(ksize, xmin [n_px], count [n_px], k [n_px, ksize]) of the block at word offset ``off``."""
        t = self.tables[off:]
        ks, n = int(t[0]), self.n_px
        return ks, t[1:1 + n], t[1 + n:1 + 2 * n], t[1 + 2 * n:1 + 2 * n + n * ks].reshape(n, ks)

    def device_tables(self, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(tables, desc, h_tiles) on ``device``; copied once per plan and device."""
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(a).to(device) for a in (self.tables, self.desc, self.h_tiles))
        return self._device[device]


_PLANS: "OrderedDict[tuple, PreprocessPlan]" = OrderedDict()
_PLAN_CACHE_SIZE = 64


def plan_for(batch: ImageBatch, n_px: int, crop_offset: str = "round") -> PreprocessPlan:
    """The plan of a batch, cached by size signature (a dataset has a handful of image sizes and a fixed batch size)."""
    if n_px <= 0:
        raise ValueError("n_px must be positive")
    key = (tuple(batch.sizes), n_px, crop_offset)
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = PreprocessPlan(batch.sizes, batch.offsets, n_px, crop_offset)
        while len(_PLANS) > _PLAN_CACHE_SIZE:
            _PLANS.popitem(last=False)
    else:
        _PLANS.move_to_end(key)
    return plan


def normalize_table(mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """float32 [3, 256]: ``ToTensor`` (uint8 -> float32, / 255) then ``Normalize`` (- mean, / std) of every byte value, computed with
    those transforms' own torch CPU ops - the kernel looks values up, so no device division decides a bit."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).reshape(-1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).reshape(-1, 1)
    if m.numel() != 3 or s.numel() != 3 or bool((s == 0).any()):
        raise ValueError("mean and std are three values each, std non-zero")
    return v.view(1, 256).repeat(3, 1).sub_(m).div_(s).contiguous()


class ClipImagePreprocessor:
    """Drop-in for ``torch.stack([image_preprocessor(im) for im in images]).to(device)``:
    ``__call__(images) -> float32 [B, 3, n_px, n_px]`` on the device, bit for bit what PIL + torchvision give on the host.
    ``crop_offset``: "round" (torchvision ``CenterCrop``, the reference) or "floor" (HF ``CLIPImageProcessor``)."""

    def __init__(self, n_px: int, mean=CLIP_MEAN, std=CLIP_STD, crop_offset: str = "round", device="cuda"):
        crop_offset_of(n_px, n_px, crop_offset)                              # rejects an unknown rule here, not at the first batch
        self.n_px, self.crop_offset, self.device = int(n_px), crop_offset, torch.device(device)
        self.lut_host = normalize_table(mean, std)
        self._lut = None

    @property
    def lut(self) -> torch.Tensor:
        if self._lut is None:
            self._lut = self.lut_host.to(self.device)
        return self._lut

    def plan(self, images) -> PreprocessPlan:
        return plan_for(as_batch(images), self.n_px, self.crop_offset)

    def _rows(self, images):
        """Host -> device copy of the packed bytes and the horizontal pass, on the current stream."""
        from .. import ops
        batch = as_batch(images)
        plan = plan_for(batch, self.n_px, self.crop_offset)
        src = batch.data.to(self.device, non_blocking=True)
        return plan, ops.clip_resize_rows(src, plan)

    def __call__(self, images) -> torch.Tensor:
        from .. import ops
        plan, mid = self._rows(images)
        return ops.clip_preprocess(mid, plan, self.lut)

    def patches(self, images, ps: int, dtype: torch.dtype, ldp: int, out=None) -> torch.Tensor:
        """The same pixels as ``ops.patchify(self(images), ps, dtype, ldp)`` - ``dtype`` ``[B * g * g, ldp]`` patch rows, pad columns
        zero - without the float32 pixel tensor in between."""
        from .. import ops
        plan, mid = self._rows(images)
        return ops.clip_preprocess_patches(mid, plan, self.lut, ps, dtype, ldp, out)
