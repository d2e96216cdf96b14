"""CPU: ``examples_from_selection`` builds the dict the reference pickles as rices.pkl (get_average_similarities.py:60-71, 97-100)."""
import numpy as np


def test_examples_from_selection_hand_table():
    from eavqa_amd.utils.rices import examples_from_selection
    # 6 train questions over 4 images; row -> question id
    train_question_ids = [1000, 1001, 2000, 3000, 3001, 4000]
    table = {
        1000: {"img_key": "img_1", "question": "what is this", "gold_answer": "cat"},
        1001: {"img_key": "img_1", "question": "what colour", "gold_answer": "black"},
        2000: {"img_key": "img_2", "question": "how many", "gold_answer": "2"},
        3000: {"img_key": "img_3", "question": "is it raining", "gold_answer": "no"},
        3001: {"img_key": "img_3", "question": "where is this", "gold_answer": "street"},
        4000: {"img_key": "img_4", "question": "what sport", "gold_answer": "tennis"},
    }
    # 3 val questions; rows as rices_select returns them: ascending score, best example last
    rows = np.array([[5, 0, 1], [2, 2, 3], [4, 3, 0]], dtype=np.int64)
    val_ids = [77001, 77002, 88000]
    out = examples_from_selection(dict(zip(val_ids, rows)), train_question_ids, table)
    assert list(out) == ["77001", "77002", "88000"]
    assert all(isinstance(k, str) for k in out)
    for v, r in zip(val_ids, rows):
        ex = out[str(v)]
        assert [e["question_id"] for e in ex] == [train_question_ids[i] for i in r]           # order kept: ascending score
        for e in ex:
            assert set(e) == {"question_id", "img_key", "question", "gold_answer"}
            src = table[e["question_id"]]
            assert (e["img_key"], e["question"], e["gold_answer"]) == (src["img_key"], src["question"], src["gold_answer"])
    assert [e["img_key"] for e in out["77001"]] == ["img_4", "img_1", "img_1"]               # img_key comes from the question's entry
    assert out["77002"][0] == out["77002"][1] == {"question_id": 2000, "img_key": "img_2", "question": "how many", "gold_answer": "2"}
    # pairs are accepted as well as a dict
    assert examples_from_selection(list(zip(val_ids, rows.tolist())), train_question_ids, table) == out
