#!/usr/bin/env python3
"""RICES end to end at VQA2 scale on seeded synthetic data (profiles/rices_end_to_end.md is this tool's output):

  * text tower: ``ClipTextEncoder.encode_text`` (ViT-L/14 text transformer, bf16, random weights) on 8 192 questions of U{4..14} tokens plus
    BOS and EOT, packed and unpacked, in questions/s;
  * text kNN: one tile of 1 024 queries against 443 757 train question embeddings x 768, k = 2048 (get_question_knn.py:64-76): the exact-fp32
    GEMM and ``eavqa_topk_rows``;
  * joint re-ranking: ``eavqa_rices_joint_scores`` for one tile of 8 192 queries, k = 2048 neighbours, 82 783 train images x 768, in us per
    query and gathered bytes per second (against 8 TB/s of HBM), then ``eavqa_topk_rows`` for n = 32;
  * the same selection with torch ops (``index_select`` + ``bmm`` + ``topk``) as a reference point only - it is never on the product path.

Every figure is the median of ``--reps`` timed runs after one warm-up, by HIP events.  ``--small`` shrinks every size (a quick functional run)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from eavqa_amd import ops  # noqa: E402
from eavqa_amd.models.clip_text import KNOWN_TEXT_TOWERS, ClipTextEncoder, random_init_text_state_dict  # noqa: E402

DEV = "cuda"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--skip-text", action="store_true")
    args = ap.parse_args()
    Ndq, Ni, D, k, n, Nq, Qknn = (443757, 82783, 768, 2048, 32, 8192, 1024) if not args.small else (20000, 4000, 768, 2048, 32, 256, 128)
    g = torch.Generator().manual_seed(2021)
    res = {"sizes": dict(train_questions=Ndq, train_images=Ni, D=D, k=k, n=n, queries=Nq, knn_tile=Qknn)}

    # ---- text tower
    if not args.skip_text:
        cfg = KNOWN_TEXT_TOWERS["ViT-L/14"]
        enc = ClipTextEncoder(cfg, random_init_text_state_dict(cfg, 2021), torch.bfloat16, DEV)
        lens = torch.randint(4, 15, (Nq,), generator=g) + 2
        ids = torch.randint(1, cfg.vocab - 2, (Nq, cfg.context), generator=g)
        ids = torch.where(torch.arange(cfg.context)[None] < lens[:, None] - 1, ids, torch.zeros_like(ids))
        ids[:, 0] = cfg.vocab - 2
        ids[torch.arange(Nq), lens - 1] = cfg.vocab - 1
        for pack in (True, False):
            ms = timed(lambda: enc.encode_text(ids, pack=pack), args.reps)
            res["encode_text_packed" if pack else "encode_text_unpacked"] = dict(ms=ms, questions_per_s=Nq / ms * 1e3,
                                                                                 rows=int(lens.sum()) if pack else Nq * cfg.context)
        del enc

    # ---- text kNN tile
    db = ops.l2_normalize_rows_(torch.randn(Ndq, D, device=DEV))
    q = ops.l2_normalize_rows_(torch.randn(Qknn, D, device=DEV))
    gemm_ms = timed(lambda: ops.gemm(q, db, out_f32=True), args.reps)
    s = ops.gemm(q, db, out_f32=True)
    topk_ms = timed(lambda: ops.topk_rows(s, k), args.reps)
    res["text_knn_tile"] = dict(queries=Qknn, gemm_ms=gemm_ms, gemm_tflops=2.0 * Qknn * Ndq * D / gemm_ms / 1e9, topk_ms=topk_ms,
                                us_per_query=(gemm_ms + topk_ms) / Qknn * 1e3)
    del db, q, s

    # ---- joint re-ranking
    train_img = ops.l2_normalize_rows_(torch.randn(Ni, D, device=DEV))
    query_img = ops.l2_normalize_rows_(torch.randn(Nq, D, device=DEV))
    text_sim = (0.3 + 0.6 * torch.rand(Nq, k, generator=g)).sort(dim=1, descending=True).values.to(DEV)
    text_idx = torch.randint(0, Ndq, (Nq, k), generator=g).to(DEV)
    q2img = torch.randint(0, Ni, (Ndq,), generator=g, dtype=torch.int32).to(DEV)
    query_row = torch.arange(Nq, dtype=torch.int32, device=DEV)
    ms = timed(lambda: ops.rices_joint_scores(text_sim, text_idx, q2img, train_img, query_img, query_row), args.reps)
    joint = ops.rices_joint_scores(text_sim, text_idx, q2img, train_img, query_img, query_row)
    sel_ms = timed(lambda: ops.topk_rows(joint, n), args.reps)
    gathered = Nq * k * D * 4
    res["joint_scores"] = dict(ms=ms, us_per_query=ms / Nq * 1e3, gathered_tb_per_s=gathered / ms / 1e9, of_8_tb_per_s=gathered / ms / 1e9 / 8.0,
                               topk_n_ms=sel_ms, topk_n_us_per_query=sel_ms / Nq * 1e3)

    def torch_selection(chunk=256):
        out = []
        for a in range(0, Nq, chunk):
            b = min(Nq, a + chunk)
            rows = q2img[text_idx[a:b].reshape(-1)].long()
            gath = train_img.index_select(0, rows).view(b - a, k, D)
            sim = torch.bmm(gath, query_img[query_row[a:b].long()].unsqueeze(2)).squeeze(2)
            out.append(torch.topk(text_sim[a:b] + sim, n, dim=1))
        return out

    t_ms = timed(torch_selection, max(1, args.reps // 2))
    res["torch_reference"] = dict(ms=t_ms, us_per_query=t_ms / Nq * 1e3)
    ref = torch.cat([o.values for o in torch_selection()])
    res["max_abs_diff_vs_torch_top_n"] = (ops.topk_rows(joint, n)[0] - ref).abs().max().item()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
