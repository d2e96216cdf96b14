"""CPU: the host plan of the CLIP image preprocessing (eavqa_amd.models.clip_preprocess) against the numpy restatement of PIL's
arithmetic in tests/_image_ref.py: coefficient tables on the cropped range, table sharing, the horizontal pass's row range, the tile
table, the normalisation table, ``ImageBatch`` packing and rejections.  No GPU, no PIL."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_ref as R  # noqa: E402

from eavqa_amd.models import clip_preprocess as P  # noqa: E402

D_SRC, D_W, D_H, D_ROW0, D_NROWS, D_MID, D_TX, D_TY = range(8)


def batch_of(n_px):
    sizes = [(H, W) for H, W, n in R.SIZES if n == n_px]
    return P.ImageBatch([R.case_image(H, W, "random") for H, W in sizes]), sizes


@pytest.mark.parametrize("rule", ["round", "floor"])
@pytest.mark.parametrize("n_px", [28, 8, 32])
def test_tables_are_the_restatements_coefficients_on_the_cropped_range(n_px, rule):
    batch, sizes = batch_of(n_px)
    plan = P.plan_for(batch, n_px, rule)
    assert plan.tables.dtype == np.int32 and plan.desc.dtype == np.int64 and plan.desc.shape == (len(sizes), 8)
    for i, (H, W) in enumerate(sizes):
        oh, ow = R.output_size(H, W, n_px)
        top, left = R.crop_box(oh, ow, n_px, rule)
        assert plan.boxes[i] == (oh, ow, top, left)
        for off, size, out, lo in ((plan.desc[i, D_TX], W, ow, left), (plan.desc[i, D_TY], H, oh, top)):
            ks, xmin, count, k = plan.table(int(off))
            ks_ref, cs = R.coeffs(size, out)
            assert ks == ks_ref
            for j in range(n_px):
                xm, kr = cs[lo + j]
                assert (int(xmin[j]), int(count[j])) == (xm, len(kr))
                assert k[j, :len(kr)].tolist() == kr and not k[j, len(kr):].any()


def test_ksize_is_not_bounded():
    ks, xmin, count, k = P.axis_table(4000, 224, 0, 224)
    assert ks == 73 and int(count.max()) <= 73 and k.shape == (224, 73)
    _, cs = R.coeffs(4000, 224)
    assert k[100, :int(count[100])].tolist() == cs[100][1]
    assert int(np.abs(k.astype(np.int64)).sum(1).max()) < 1.4 * 2 ** 22       # int32 sums suffice: 255 * 1.4 * 2^22 + 2^21 < 2^31


def test_tables_are_shared_between_equal_in_out_pairs_and_plans_are_cached():
    imgs = [R.case_image(H, W, "random") for H, W in ((48, 64), (48, 64), (64, 48), (48, 80))]
    batch = P.ImageBatch(imgs)
    plan = P.plan_for(batch, 28)
    d = plan.desc
    assert d[0, D_TX] == d[1, D_TX] and d[0, D_TY] == d[1, D_TY]
    assert d[0, D_TY] == d[3, D_TY] and d[0, D_TX] != d[3, D_TX]              # 48 -> 28 rows shared, the columns differ
    assert len(plan.table_offset) == 5                                        # x: (64, 37), (48, 28), (80, 46); y: (48, 28), (64, 37)
    assert sorted(plan.table_offset) == [(0, 48, 28), (0, 64, 37), (1, 48, 28), (1, 64, 37), (1, 80, 46)]
    words = sum(1 + 2 * 28 + 28 * plan.table(o)[0] for o in plan.table_offset.values())
    assert plan.tables.size == words
    assert P.plan_for(P.ImageBatch(imgs), 28) is plan                         # same size signature
    assert P.plan_for(batch, 28, "floor") is not plan and P.plan_for(batch, 14) is not plan


@pytest.mark.parametrize("n_px", [28, 8, 32])
def test_horizontal_row_range_is_what_the_vertical_windows_read(n_px):
    batch, sizes = batch_of(n_px)
    plan = P.plan_for(batch, n_px)
    mid = 0
    for i, (H, W) in enumerate(sizes):
        oh, ow = R.output_size(H, W, n_px)
        top, _ = R.crop_box(oh, ow, n_px)
        _, cs = R.coeffs(H, oh)
        read = set()
        for y in range(top, top + n_px):
            read |= set(range(cs[y][0], cs[y][0] + len(cs[y][1])))
        row0, nrows = int(plan.desc[i, D_ROW0]), int(plan.desc[i, D_NROWS])
        assert (row0, row0 + nrows) == (min(read), max(read) + 1) and 0 <= row0 and row0 + nrows <= H
        assert int(plan.desc[i, D_MID]) == mid and mid % 4 == 0
        assert (int(plan.desc[i, D_SRC]), int(plan.desc[i, D_W]), int(plan.desc[i, D_H])) == (int(batch.offsets[i]), W, H)
        mid += nrows * plan.mid_stride
    assert plan.mid_bytes == mid and plan.mid_stride % 4 == 0 and plan.mid_stride >= 3 * n_px
    assert plan.src_bytes == batch.nbytes == sum(H * W * 3 for H, W in sizes)
    # a crop that drops rows also drops them from the horizontal pass: 333 x 37 -> 8 keeps the middle of 72 output rows
    if n_px == 8:
        i = sizes.index((333, 37))
        assert int(plan.desc[i, D_NROWS]) < 333 // 4


@pytest.mark.parametrize("n_px", [28, 8, 32])
def test_tile_table_covers_every_row_once(n_px):
    batch, sizes = batch_of(n_px)
    plan = P.plan_for(batch, n_px)
    assert plan.h_tiles.dtype == np.int32 and plan.h_tiles.shape[1] == 2
    seen = [np.zeros(int(n), dtype=np.int64) for n in plan.desc[:, D_NROWS]]
    for img, r0 in plan.h_tiles.tolist():
        assert r0 % P.H_TILE_ROWS == 0 and 0 <= r0 < len(seen[img])
        seen[img][r0:r0 + P.H_TILE_ROWS] += 1
    assert all((s == 1).all() for s in seen)
    assert any(len(s) > P.H_TILE_ROWS for s in seen) or n_px == 8            # more than one tile per image somewhere
    assert P.V_TILE_ROWS == 4 and P.H_TILE_ROWS == 16                         # csrc/image.hip: IMG_V_TILE, IMG_H_TILE


def test_plan_reproduces_the_restatement_when_executed_in_numpy():
    """The tables, descriptors and tiles ARE the computation: running them with plain integer numpy gives the restatement's bytes."""
    n_px = 8
    batch, sizes = batch_of(n_px)
    for rule in ("round", "floor"):
        plan = P.plan_for(batch, n_px, rule)
        src = batch.data.numpy().astype(np.int64)
        mid = np.zeros(plan.mid_bytes, dtype=np.int64)
        for img, r0 in plan.h_tiles.tolist():
            so, W, H, row0, nrows, mo, tx, _ = plan.desc[img].tolist()
            ks, xmin, count, k = plan.table(tx)
            for r in range(r0, min(r0 + P.H_TILE_ROWS, nrows)):
                row = src[so + (row0 + r) * W * 3: so + (row0 + r + 1) * W * 3].reshape(W, 3)
                for x in range(n_px):
                    acc = (1 << 21) + (row[xmin[x]:xmin[x] + count[x]] * k[x, :count[x], None].astype(np.int64)).sum(0)
                    mid[mo + r * plan.mid_stride + 3 * x: mo + r * plan.mid_stride + 3 * x + 3] = np.clip(acc >> 22, 0, 255)
        for i, (H, W) in enumerate(sizes):
            _, _, _, row0, nrows, mo, _, ty = plan.desc[i].tolist()
            ks, ymin, count, k = plan.table(ty)
            rows = mid[mo:mo + nrows * plan.mid_stride].reshape(nrows, plan.mid_stride)[:, :3 * n_px]
            out = np.stack([np.clip(((1 << 21) + (rows[ymin[y] - row0:ymin[y] - row0 + count[y]] * k[y, :count[y], None].astype(np.int64)).sum(0)) >> 22,
                                    0, 255) for y in range(n_px)]).reshape(n_px, n_px, 3)
            assert np.array_equal(out, R.resize_crop_u8(batch.image(i), n_px, rule)), (sizes[i], rule)


def test_normalize_table_is_totensor_then_normalize():
    lut = P.normalize_table()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
    assert np.array_equal(lut.numpy(), R.normalize_table())
    for c in range(3):
        want = (torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255) - torch.tensor(R.CLIP_MEAN[c])) / torch.tensor(R.CLIP_STD[c])
        assert torch.equal(lut[c], want)
    other = P.normalize_table((0.5, 0.5, 0.5), (0.5, 0.25, 0.125))
    assert other[0, 255].item() == 1.0 and other[2, 0].item() == -4.0
    with pytest.raises(ValueError):
        P.normalize_table((0.5, 0.5), (1.0, 1.0))
    with pytest.raises(ValueError):
        P.normalize_table(std=(1.0, 0.0, 1.0))


def test_image_batch_packs_one_contiguous_buffer():
    imgs = [R.case_image(3, 5, "random"), R.case_image(20, 13, "checker"), R.case_image(1, 1, "random")]
    b = P.ImageBatch(imgs)
    assert len(b) == 3 and b.sizes == [(3, 5), (20, 13), (1, 1)] and b.offsets.tolist() == [0, 45, 45 + 780]
    assert b.data.dtype == torch.uint8 and b.data.is_contiguous() and b.data.numel() == b.nbytes == 45 + 780 + 3
    for i, im in enumerate(imgs):
        assert np.array_equal(b.image(i), im)
    assert P.as_batch(b) is b
    # a non-contiguous view and a torch tensor are packed by value
    wide = R.case_image(6, 10, "random")
    b2 = P.ImageBatch([wide[::2, ::2], torch.from_numpy(wide)])
    assert np.array_equal(b2.image(0), wide[::2, ::2]) and np.array_equal(b2.image(1), wide)


def test_image_batch_accepts_pil_images():
    Image = pytest.importorskip("PIL.Image")
    a = R.case_image(7, 9, "random")
    assert np.array_equal(P.ImageBatch([Image.fromarray(a)]).image(0), a)


@pytest.mark.parametrize("bad,exc", [
    ([np.zeros((4, 4, 3), dtype=np.float32)], TypeError),
    ([np.zeros((4, 4, 3), dtype=np.int16)], TypeError),
    ([np.zeros((4, 4, 4), dtype=np.uint8)], ValueError),
    ([np.zeros((4, 4), dtype=np.uint8)], ValueError),
    ([np.zeros((4, 4, 1), dtype=np.uint8)], ValueError),
    ([np.zeros((0, 4, 3), dtype=np.uint8)], ValueError),
    ([np.zeros((4, 0, 3), dtype=np.uint8)], ValueError),
    ([np.zeros((4, 4, 3), dtype=np.uint8), np.zeros((4, 4, 3), dtype=np.float64)], TypeError),
    ([], TypeError),
    (np.zeros((2, 4, 4, 3), dtype=np.uint8), TypeError),
], ids=["float32", "int16", "rgba", "gray2d", "one-channel", "zero-rows", "zero-columns", "second-image", "empty-list", "stacked-array"])
def test_image_batch_rejections(bad, exc):
    with pytest.raises(exc):
        P.ImageBatch(bad)


def test_preprocessor_rejects_an_unknown_crop_rule_and_size():
    with pytest.raises(ValueError):
        P.ClipImagePreprocessor(28, crop_offset="ceil", device="cpu")
    with pytest.raises(ValueError):
        P.plan_for(P.ImageBatch([R.case_image(4, 4, "random")]), 0)
    pre = P.ClipImagePreprocessor(28, device="cpu")
    assert pre.plan([R.case_image(48, 64, "random")]).boxes == [(28, 37, 0, 4)]       # round(4.5) = 4: half to even
    assert P.ClipImagePreprocessor(28, crop_offset="floor", device="cpu").plan([R.case_image(61, 28, "random")]).boxes == [(61, 28, 16, 0)]
