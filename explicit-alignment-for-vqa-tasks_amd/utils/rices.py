"""RICES: retrieval of in-context examples by CLIP-embedding similarity, on the GPU.

Mirror of src/in_context_example_selection/get_question_knn.py:64-76 - ``faiss.normalize_L2`` on the
database (train question embeddings) and on the queries (val question embeddings), ``IndexFlatIP`` search with
``k = 2048`` - as three HIP steps per tile of queries: exact-fp32 MFMA GEMM for the inner products, then a
radix-select top-k (``eavqa_topk_rows``).  Returns faiss's ``(D, I)``: similarities sorted descending and int64 row
numbers into the database.

faiss is not installed here and the reference ships no retrieval outputs, so index-for-index parity with faiss is
*unpinned*: scores are exact fp32 sums in a different order than faiss's BLAS call, and among exactly equal scores this
build returns the smaller database row first (faiss leaves that order unspecified).  tests/test_retrieval_gpu.py pins the
kernels against float64 numpy instead.

``rices_select`` is the rest of the reference's selection, on the GPU: the image k-NN among the text neighbours
(get_image_knn_from_text_knn.py:59-92: the 2048 question neighbours mapped to their images, de-duplicated, a fresh faiss index per
val question searched with that question's image) and the merge (get_average_similarities.py:46-71: ``joint = image similarity +
question similarity`` on ``img_key``, ``nlargest(32)`` sorted ascending) collapse into one formula per text neighbour j of query i,

    joint[i, j] = text_sim[i, j] + <val_img[i], train_img[image_of_question[text_idx[i, j]]]>,

one gather-and-dot kernel (``eavqa_rices_joint_scores``) and one ``eavqa_topk_rows`` over ``joint``.  The text embeddings come from
``models/clip_text.py``; reading the VQA2 files and the CLIP tokeniser stay with the caller.

Deviation from the reference, on purpose: pandas ``nlargest(32, keep="all")`` returns MORE than 32 rows when the 32nd value is tied;
this build returns exactly ``n`` and breaks ties by text rank (the better text neighbour first).  Parity with the reference's
``rices.pkl`` is unpinned for the same reason as the k-NN above (no faiss, no pandas, no shipped outputs);
tests/test_rices_rerank_gpu.py pins the selection to a float64 restatement.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

from .. import ops

Tensor = torch.Tensor


def knn_inner_product(database: Tensor, queries: Tensor, k: int = 2048, normalize: bool = True,
                      query_tile: int = 1024) -> Tuple[Tensor, Tensor]:
    """``database`` [Nd, D], ``queries`` [Nq, D] float32 on the GPU (the reference stacks ``[1, D]`` pickled entries and
    squeezes, get_question_knn.py:45,60).  ``normalize=True`` works on copies.  Peak extra memory: one
    ``[query_tile, Nd]`` float32 score tile (1.8 GB at Nd = 443 k)."""
    if database.dim() != 2 or queries.dim() != 2 or database.shape[1] != queries.shape[1]:
        raise ValueError("knn_inner_product: database [Nd, D] and queries [Nq, D] expected")
    if not 0 < k <= min(2048, database.shape[0]):
        raise ValueError("knn_inner_product: 1 <= k <= min(2048, Nd)")
    db = database.to(torch.float32).contiguous()
    q = queries.to(torch.float32).contiguous()
    if normalize:
        db = ops.l2_normalize_rows_(db.clone() if db.data_ptr() == database.data_ptr() else db)
        q = ops.l2_normalize_rows_(q.clone() if q.data_ptr() == queries.data_ptr() else q)
    Nq = q.shape[0]
    D = torch.empty((Nq, k), device=q.device, dtype=torch.float32)
    I = torch.empty((Nq, k), device=q.device, dtype=torch.int64)
    for s in range(0, Nq, query_tile):
        e = min(Nq, s + query_tile)
        scores = ops.gemm(q[s:e], db, out_f32=True)
        D[s:e], I[s:e] = ops.topk_rows(scores, k)
    return D, I


def rices_neighbours(train_embeddings: Tensor, val_embeddings: Tensor, k: int = 2048) -> Tuple[Tensor, Tensor]:
    """The two arrays the reference saves (``text_nearest_neighbours_similarities_2048.npy`` = D,
    ``text_nearest_neighbours_2048.npy`` = I, get_question_knn.py:78-81)."""
    return knn_inner_product(train_embeddings, val_embeddings, k=k, normalize=True)


def rices_select(train_text: Tensor, val_text: Tensor, train_img: Tensor, val_img: Tensor, q2img: Tensor, val_query_row: Tensor,
                 n: int = 32, k: int = 2048, question_only: bool = False, query_tile: int = 1024,
                 normalize: bool = True) -> Tuple[Tensor, Tensor]:
    """In-context examples of every val question: ``(scores float32 [Nq, n], question_rows int64 [Nq, n])``, rows into
    ``train_text``, ASCENDING in score as the reference's ``sort_values`` leaves them (the best example last).

    ``train_text`` [Ndq, D] / ``val_text`` [Nq, D]: CLIP text embeddings of the train / val questions; ``train_img`` [Ni, Di] /
    ``val_img`` [Nqi, Di]: CLIP image embeddings; ``q2img`` int [Ndq]: train question row -> train image row; ``val_query_row`` int
    [Nq]: val question row -> row of ``val_img``.  All four matrices are L2-normalised on copies, once (``normalize=False``: they
    already are).  ``question_only=True`` is the
    reference's ``rices_questions_only`` variant (get_average_similarities.py:73-93): the first ``n`` text neighbours."""
    if not 0 < n <= k:
        raise ValueError("rices_select: 1 <= n <= k")
    dev = train_text.device

    def norm(m: Tensor) -> Tensor:
        m32 = m.to(device=dev, dtype=torch.float32).contiguous()
        if not normalize:
            return m32
        return ops.l2_normalize_rows_(m32.clone() if m32.data_ptr() == m.data_ptr() else m32)

    tt, vt = norm(train_text), norm(val_text)
    Nq = vt.shape[0]
    if not question_only:
        ti, vi = norm(train_img), norm(val_img)
        q2img = q2img.to(device=dev, dtype=torch.int32).contiguous()
        val_query_row = val_query_row.to(device=dev, dtype=torch.int32).contiguous()
        if q2img.numel() != tt.shape[0] or val_query_row.numel() != Nq:
            raise ValueError("rices_select: q2img has one entry per train question, val_query_row one per val question")
    scores = torch.empty((Nq, n), device=dev, dtype=torch.float32)
    rows = torch.empty((Nq, n), device=dev, dtype=torch.int64)
    for s in range(0, Nq, query_tile):
        e = min(Nq, s + query_tile)
        D, I = knn_inner_product(tt, vt[s:e], k=k, normalize=False, query_tile=query_tile)
        if question_only:
            top, pick = D[:, :n], I[:, :n]
        else:
            joint = ops.rices_joint_scores(D, I, q2img, ti, vi, val_query_row[s:e])
            top, col = ops.topk_rows(joint, n)                     # ties: the smaller column = the better text rank
            pick = torch.gather(I, 1, col)
        scores[s:e], rows[s:e] = top.flip(1), pick.flip(1)
    return scores, rows


def examples_from_selection(question_rows, train_question_ids: Sequence, vqa2_data_by_q_id: Dict) -> Dict[str, List[dict]]:
    """The dict the reference pickles (get_average_similarities.py:60-71, 97-100): ``{str(val_question_id): [example, ...]}`` with
    ``example = {question_id, img_key, question, gold_answer}`` taken from the train question's entry, in the order of
    ``question_rows`` (ascending score).  ``question_rows``: ``{val_question_id: row numbers}`` or a sequence of
    ``(val_question_id, row numbers)`` pairs, row numbers into ``train_question_ids``.  Pure host code."""
    items = question_rows.items() if hasattr(question_rows, "items") else question_rows
    out: Dict[str, List[dict]] = {}
    for val_id, rows_of in items:
        examples = []
        for r in (rows_of.tolist() if hasattr(rows_of, "tolist") else rows_of):
            qid = train_question_ids[int(r)]
            entry = vqa2_data_by_q_id[int(qid)]
            examples.append({"question_id": qid, "img_key": entry["img_key"], "question": entry["question"],
                             "gold_answer": entry["gold_answer"]})
        out[str(val_id)] = examples
    return out
