"""CPU checks of the doc-view / similar-pages boundary: the numpy model (tests/doc_view_model.py) on hand-worked cases, and the new
entry points in the header, the ctypes binding and the engine wrappers (no compute calls — there is no GPU here)."""
import os
import re

import numpy as np

from tests import doc_view_model as dvm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
NEW = ("ss_index_build_doc_view", "ss_index_drop_doc_view", "ss_index_read_doc_view", "ss_index_doc_top_terms", "ss_similar_topk")


def tiny_body():
    """the body table of tests/test_gpu_score.py::tiny_index (importing that module needs no GPU)"""
    from tests.test_gpu_score import tiny_index
    return tiny_index()[1]


def test_view_of_the_tiny_index_by_hand():
    dp, dt, dw = dvm.doc_view(*tiny_body(), 5)
    assert dp.dtype == np.uint64 and dt.dtype == np.uint32 and dw.dtype == np.float32
    assert dp.tolist() == [0, 1, 3, 4, 5, 6]
    assert dt.tolist() == [0, 0, 1, 0, 1, 2]                 # doc 1 holds terms 0 and 1
    assert dw.tolist() == [1.0, 2.0, 4.0, 0.5, 1.0, 3.0]     # ... with weights {0: 2.0, 1: 4.0}
    terms, w, n = dvm.top_terms((dp, dt, dw), [1, 1, 4, 0], 1)
    assert terms[:, 0].tolist() == [1, 1, 2, 0] and w[:, 0].tolist() == [4.0, 4.0, 3.0, 1.0] and n.tolist() == [1, 1, 1, 1]
    terms, w, n = dvm.top_terms((dp, dt, dw), [1, 2], 5)
    assert n.tolist() == [2, 1] and terms[0].tolist() == [1, 0, 0, 0, 0] and w[0].tolist() == [4.0, 2.0, 0, 0, 0]
    assert terms[1].tolist() == [0, 0, 0, 0, 0]
    # a doc beyond every posting and an empty table
    dp6, _, _ = dvm.doc_view(*tiny_body(), 7)
    assert dp6.tolist() == [0, 1, 3, 4, 5, 6, 6, 6]
    e = dvm.doc_view(np.zeros(4, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 3)
    assert e[0].tolist() == [0, 0, 0, 0] and len(e[1]) == 0


def one_row(weights):
    """a table in which doc 0 holds term t with weights[t]"""
    T = len(weights)
    return dvm.doc_view(np.arange(T + 1, dtype=np.uint64), np.zeros(T, np.uint32), np.array(weights, np.float32), 1)


def test_order_of_top_terms():
    nan, inf = float("nan"), float("inf")
    # a weight tie: ascending term id
    t, w, n = dvm.top_terms(one_row([1.0, 3.0, 3.0, 0.5, 3.0]), [0], 5)
    assert t[0].tolist() == [1, 2, 4, 0, 3]
    # -0.0 and +0.0 are one weight: the term decides, and the stored bits come back
    t, w, n = dvm.top_terms(one_row([-1.0, 0.0, -0.0, 0.0, -0.0, 1.0]), [0], 6)
    assert t[0].tolist() == [5, 1, 2, 3, 4, 0]
    assert np.signbit(w[0]).tolist() == [False, False, True, False, True, True]
    # NaN last, NaNs by term; +Inf first, -Inf behind every finite weight; negatives by value
    t, w, n = dvm.top_terms(one_row([nan, -2.0, inf, -inf, nan, -0.5, 7.0, 0.0]), [0], 8)
    assert t[0].tolist() == [2, 6, 7, 5, 1, 3, 0, 4] and n.tolist() == [8]
    assert np.isnan(w[0, 6:]).all() and w[0, 0] == inf and w[0, 5] == -inf
    t, w, n = dvm.top_terms(one_row([nan, -2.0, inf, -inf, nan, -0.5, 7.0, 0.0]), [0], 3)
    assert t[0].tolist() == [2, 6, 7] and n.tolist() == [3]


def test_drop_seed_and_queries():
    from spaghettisearch_amd import engine
    rows = np.zeros((3, 4), dtype=engine.HIT_DTYPE)
    rows["doc"] = [[5, 6, 7, 8], [1, 2, 3, 0], [9, 0, 0, 0]]
    rows["final"] = [[4, 3, 2, 1], [4, 3, 2, 0], [1, 0, 0, 0]]
    out, n = dvm.drop_seed(rows, np.array([4, 3, 1]), [6, 9, 9], 3)
    assert n.tolist() == [3, 3, 0]
    assert out["doc"].tolist() == [[5, 7, 8], [1, 2, 3], [0, 0, 0]] and out["final"][0].tolist() == [4, 2, 1]
    out, n = dvm.drop_seed(rows, np.array([4, 3, 1]), [0, 1, 3], 3)          # seed not in the row: the first k rows
    assert out["doc"].tolist() == [[5, 6, 7], [2, 3, 0], [9, 0, 0]] and n.tolist() == [3, 2, 1]
    q_ptr, q_terms = dvm.queries_of(np.array([[3, 1], [0, 0], [2, 0]], np.uint32), np.array([2, 0, 1], np.int32))
    assert q_ptr.tolist() == [0, 2, 2, 3] and q_terms.tolist() == [3, 1, 2]


def test_header_declares_the_new_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", text), name
    m = re.search(r"ss_similar_topk\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(m.group(1).split(",")) == 9
    m = re.search(r"ss_index_doc_top_terms\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert len(m.group(1).split(",")) == 7
    assert re.search(r"#define SS_ABI_VERSION 4\b", text)


def test_binding_and_engine_expose_them():
    from spaghettisearch_amd import _lib, engine
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["ss_similar_topk"][1]) == 9 and len(_lib.PROTOTYPES["ss_index_doc_top_terms"][1]) == 7
    for meth in ("build_doc_view", "drop_doc_view", "read_doc_view", "doc_top_terms"):
        assert callable(getattr(engine.InvertedIndex, meth))
    assert callable(engine.Scorer.similar_topk)
    import inspect
    sig = inspect.signature(engine.Scorer.similar_topk)
    assert list(sig.parameters)[1:] == ["seeds", "k", "m", "topic_probs", "mask_id", "out"] and sig.parameters["m"].default == 5
    assert inspect.signature(engine.InvertedIndex.doc_top_terms).parameters["want_w"].default is True
