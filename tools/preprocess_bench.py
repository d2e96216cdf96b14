#!/usr/bin/env python3
"""CLIP image preprocessing: the few-shot batch of BASELINE configs[3] - 160 raw images of 640x480 - to n_px 224 (ViT-L/14) and 336
(ViT-L/14@336px, the README's tower row), on the card against today's host route.

Per n_px, REPS rounds after WARMUP ones, in every round one pass of each route in turn (drift of the box hits both alike), medians:
  new route   the host -> device copy of the packed uint8 batch (pinned, one copy), eavqa_clip_resize_rows, eavqa_clip_resize_emit as
              float32 NCHW and as bf16 patch rows - each between two device events - and ``encode_raw`` end to end (random-init tower,
              bf16) next to ``encode_image`` on pixels that are already on the card;
  baseline    what a user of the parent does: PIL ``resize(BICUBIC)`` + ``crop`` + ToTensor / Normalize per image on THREADS host threads
              (wall clock), ``torch.stack`` and the float32 host -> device copy (wall clock around a synchronise).  Never the code under test.
Roofline: each kernel's bytes by the byte model (the source read once by the horizontal pass, the intermediate written once and read
once, the output written once - computed here from the plan) over its time, next to the 6.29 TB/s streaming-copy rate of the MI355X.
Writes the markdown table to --out and prints one JSON object as the last line.

    python tools/preprocess_bench.py --out profiles/clip_preprocess.md
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eavqa_amd import ops
from eavqa_amd.models.clip_preprocess import CLIP_MEAN, CLIP_STD, ClipImagePreprocessor, ImageBatch, crop_offset_of, output_size
from eavqa_amd.models.clip_vit import ClipVisionEncoder, ViTConfig, random_init_vit_state_dict

COPY_RATE = 6.29e12          # bytes / s, streaming copy on the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=160)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--n-px", type=int, nargs="+", default=[224, 336])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--layers", type=int, default=24, help="tower depth (24 = ViT-L/14)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("preprocess_bench.py measures on the GPU; there is none here")
try:
    from PIL import Image
except ImportError:                                   # the baseline is then reported as not measured, never replaced by something else
    Image = None

dev = "cuda:0"
rng = np.random.RandomState(2021)
images = [rng.randint(0, 256, (args.height, args.width, 3), dtype=np.uint8) for _ in range(args.images)]
mean = torch.as_tensor(CLIP_MEAN, dtype=torch.float32).view(3, 1, 1)
std = torch.as_tensor(CLIP_STD, dtype=torch.float32).view(3, 1, 1)


def timed(fn):
    """(milliseconds between two device events around fn, its result)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_one(img, n_px):
    oh, ow = output_size(img.shape[0], img.shape[1], n_px)
    top, left = crop_offset_of(oh, n_px, "round"), crop_offset_of(ow, n_px, "round")
    im = Image.fromarray(img).resize((ow, oh), Image.BICUBIC).crop((left, top, left + n_px, top + n_px))
    t = torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return t.sub_(mean).div_(std)


results, lines = {}, []
pool = ThreadPoolExecutor(max_workers=args.threads)
for n_px in args.n_px:
    pre = ClipImagePreprocessor(n_px, device=dev)
    batch = ImageBatch(images)
    plan = pre.plan(batch)
    vcfg = ViTConfig(1024, args.layers, 16, 4096, 14, n_px, 768)
    vit = ClipVisionEncoder(vcfg, random_init_vit_state_dict(vcfg, 5, dev), torch.bfloat16, dev)
    out_bytes = args.images * 3 * n_px * n_px * 4
    g = n_px // 14
    patch_bytes = args.images * g * g * vit.kpad * 2
    model = dict(rows=plan.src_bytes + plan.mid_bytes, emit_nchw=plan.mid_bytes + out_bytes, emit_patches=plan.mid_bytes + patch_bytes)
    t = {k: [] for k in ("h2d_u8", "rows", "emit_nchw", "emit_patches", "encode_raw", "encode_image", "host_pil", "host_stack_h2d")}
    for it in range(args.warmup + args.reps):
        keep = it >= args.warmup
        rec = {}
        if Image is not None:
            t0 = time.perf_counter()
            host = list(pool.map(lambda im: host_one(im, n_px), images))
            rec["host_pil"] = (time.perf_counter() - t0) * 1e3
            rec["host_stack_h2d"], host_px = wall(lambda: torch.stack(host).to(dev))
        rec["h2d_u8"], src = timed(lambda: batch.data.to(dev, non_blocking=True))
        rec["rows"], mid = timed(lambda: ops.clip_resize_rows(src, plan))
        rec["emit_nchw"], px = timed(lambda: ops.clip_preprocess(mid, plan, pre.lut))
        rec["emit_patches"], _ = timed(lambda: ops.clip_preprocess_patches(mid, plan, pre.lut, 14, torch.bfloat16, vit.kpad))
        rec["encode_raw"], emb = wall(lambda: vit.encode_raw(batch))
        rec["encode_image"], emb2 = wall(lambda: vit.encode_image(px))
        if it == 0:
            assert torch.equal(emb, emb2), "encode_raw differs from encode_image(preprocessor(images))"
            if Image is not None:
                assert torch.equal(px, host_px), "the card's pixels differ from PIL's"
        if keep:
            for k, v in rec.items():
                t[k].append(v)
    med = {k: (statistics.median(v) if v else None) for k, v in t.items()}
    spread = {k: ((min(v), max(v)) if v else None) for k, v in t.items()}
    rate = {k: model[k] / (med[k] * 1e-3) for k in model}
    results[n_px] = dict(median_ms=med, min_max_ms=spread, model_bytes=model, bytes_per_s=rate,
                         share_of_copy_rate={k: rate[k] / COPY_RATE for k in rate}, src_bytes=plan.src_bytes, mid_bytes=plan.mid_bytes,
                         f32_pixel_bytes=out_bytes, taps=(plan.table(int(plan.desc[0, 6]))[0], plan.table(int(plan.desc[0, 7]))[0]))
    f = lambda k: "not measured" if med[k] is None else f"{med[k]:.3f} ({spread[k][0]:.3f} - {spread[k][1]:.3f})"
    lines += [
        f"### {args.images} images {args.width}x{args.height} -> {n_px} (taps x / y: {results[n_px]['taps'][0]} / {results[n_px]['taps'][1]})", "",
        "| stage | median ms (min - max) | bytes (model) | achieved | share of 6.29 TB/s |", "|---|---|---|---|---|",
        f"| host -> device copy, uint8 batch (pinned) | {f('h2d_u8')} | {plan.src_bytes / 1e6:.1f} MB | {plan.src_bytes / (med['h2d_u8'] * 1e-3) / 1e9:.1f} GB/s | - |",
    ]
    for k, label in (("rows", "`eavqa_clip_resize_rows` (horizontal pass)"), ("emit_nchw", "`eavqa_clip_resize_emit`, float32 NCHW"),
                     ("emit_patches", "`eavqa_clip_resize_emit`, bf16 patch rows")):
        lines.append(f"| {label} | {f(k)} | {model[k] / 1e6:.1f} MB | {rate[k] / 1e12:.3f} TB/s | {100 * rate[k] / COPY_RATE:.1f} % |")
    lines += [
        f"| `encode_raw` end to end (copy + both kernels + tower, wall) | {f('encode_raw')} | | | |",
        f"| `encode_image` on device pixels (tower alone, wall) | {f('encode_image')} | | | |",
        f"| baseline: PIL resize + crop + normalise, {args.threads} host threads (wall) | {f('host_pil')} | | | |",
        f"| baseline: `torch.stack` + float32 host -> device copy (wall) | {f('host_stack_h2d')} | {out_bytes / 1e6:.1f} MB | | |", "",
    ]
    del vit
    torch.cuda.empty_cache()

text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
print(json.dumps(dict(tool="preprocess_bench", images=args.images, size=[args.height, args.width], reps=args.reps, threads=args.threads,
                      pil=Image is not None, results=results)))
