"""CPU checks of "related terms" (ss_related_terms): the numpy model (tests/related_terms_model.py) on a hand-worked table, the
order clause of its float64 sums, and the new entry point in the header, the built library, the ctypes binding and the engine
wrapper (no compute calls — there is no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np

from tests import doc_view_model as dvm
from tests import related_terms_model as rtm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")


def table_of(doc_rows, n_terms):
    """doc_rows: one {term: weight} per doc -> the term-major table (term_ptr, post_doc, post_w)"""
    lists = [[(d, row[t]) for d, row in enumerate(doc_rows) if t in row] for t in range(n_terms)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    doc = np.array([d for x in lists for d, _ in x], dtype=np.uint32)
    w = np.array([v for x in lists for _, v in x], dtype=np.float32)
    return ptr, doc, w


def hits_of(rows_docs, k_fb):
    """lists of doc ids -> (rows [n_q][k_fb] HIT_DTYPE, n_rows); slots behind a row's last hit name doc 2, a doc WITH postings: the
    model must ignore them by their index"""
    from spaghettisearch_amd import engine
    rows = np.zeros((len(rows_docs), k_fb), dtype=engine.HIT_DTYPE)
    rows["doc"] = 2
    for q, docs in enumerate(rows_docs):
        rows["doc"][q, :len(docs)] = docs
    return rows, np.array([len(d) for d in rows_docs], dtype=np.int32)


# six docs, eight terms; doc 3 has no body posting
HAND_DOCS = [{0: 4.0, 1: 2.0, 2: 1.0}, {0: 1.0, 1: 3.0, 3: 3.0}, {2: 2.0, 3: 0.5, 4: 5.0}, {}, {0: 2.0, 5: 1.0}, {6: 1.0, 7: 1.0}]


def test_hand_worked_rows():
    view = dvm.doc_view(*table_of(HAND_DOCS, 8), 6)
    rows, n_rows = hits_of([[0, 1, 3, 2], [5], [], [4, 0]], 4)
    q_ptr = np.array([0, 1, 3, 4, 5], dtype=np.uint32)
    q_terms = np.array([0, 6, 7, 1, 5], dtype=np.uint32)
    # query 0 typed term 0; with m_doc = 2 its hits give  doc 0: (0, 4.0) (1, 2.0)   doc 1: (1, 3.0) (3, 3.0) [a weight tie: term 1
    # first]   doc 3: nothing   doc 2: (4, 5.0) (2, 2.0).  Sums: 1 -> 5.0, 3 -> 3.0, 4 -> 5.0, 2 -> 2.0; terms 1 and 4 tie: the id decides.
    # query 1 typed 6 and 7, all its only hit holds.  query 2 has no hits.  query 3 typed 5: doc 4: (0, 2.0) (5, 1.0), doc 0: (0, 4.0) (1, 2.0).
    terms, score, n = rtm.related_ref(rows, n_rows, view, q_ptr, q_terms, 2, 3)
    assert terms.dtype == np.uint32 and score.dtype == np.float64 and n.dtype == np.int32
    assert n.tolist() == [3, 0, 0, 2]
    assert terms.tolist() == [[1, 4, 3], [0, 0, 0], [0, 0, 0], [0, 1, 0]]
    assert score.tolist() == [[5.0, 5.0, 3.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [6.0, 2.0, 0.0]]
    # m larger than the candidate count
    terms, score, n = rtm.related_ref(rows, n_rows, view, q_ptr, q_terms, 2, 8)
    assert n.tolist() == [4, 0, 0, 2]
    assert terms[0].tolist() == [1, 4, 3, 2, 0, 0, 0, 0] and score[0].tolist() == [5.0, 5.0, 3.0, 2.0, 0, 0, 0, 0]
    # m_doc = 1: every hit gives its heaviest term only; query 3's hits both give the term 0
    terms, score, n = rtm.related_ref(rows, n_rows, view, q_ptr, q_terms, 1, 3)
    assert n.tolist() == [2, 0, 0, 1]
    assert terms[0, :2].tolist() == [4, 1] and score[0, :2].tolist() == [5.0, 3.0] and terms[3, 0] == 0 and score[3, 0] == 6.0


def test_candidate_order():
    nan, inf = float("nan"), float("inf")
    assert rtm.candidate_order([7, 3, 5, 1, 2, 9, 4], [nan, -0.0, 0.0, nan, -inf, inf, 1e-300]) == [5, 6, 1, 2, 4, 3, 0]


def test_sum_order_is_not_vacuous():
    """1e-12, 1e3, -1e3 as float32, summed in float64: in rank order the small addend is rounded at 1e3's exponent before 1e3 goes
    again; with the large ones first it survives exactly."""
    w = [np.float32(1e-12), np.float32(1e3), np.float32(-1e3)]
    in_order = rtm.sum_in_order(w)
    permuted = rtm.sum_in_order([w[1], w[2], w[0]])
    assert permuted == np.float64(np.float32(1e-12))
    assert in_order != permuted and in_order.tobytes() != permuted.tobytes()
    assert in_order == (np.float64(w[0]) + np.float64(1e3)) - np.float64(1e3)
    # through the model: three hits hold term 0 with these weights, in this rank order and in the other
    docs = [{0: w[0], 1: 9.0}, {0: w[1], 1: 9.0}, {0: w[2], 1: 9.0}]
    view = dvm.doc_view(*table_of(docs, 2), 3)
    q_ptr, q_terms = np.array([0, 1, 2], np.uint32), np.array([1, 1], np.uint32)
    rows, n_rows = hits_of([[0, 1, 2], [1, 2, 0]], 3)
    terms, score, n = rtm.related_ref(rows, n_rows, view, q_ptr, q_terms, 2, 4)
    assert n.tolist() == [1, 1] and terms[:, 0].tolist() == [0, 0]
    assert score[0, 0].tobytes() == in_order.tobytes() and score[1, 0].tobytes() == permuted.tobytes()
    # a sum starts from 0.0: a lone -0.0 weight gives +0.0
    assert not np.signbit(rtm.sum_in_order([np.float32(-0.0)])) and np.signbit(np.float64(np.float32(-0.0)))


def test_header_library_binding_and_engine_have_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+SS_MAX_FEEDBACK_DOCS\s+64\b", text)
    m = re.search(r"\bint32_t\s+ss_related_terms\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == 13
    assert re.search(r"#define SS_ABI_VERSION 4\b", text)
    abi_comment = raw[:raw.index("#define SS_ABI_VERSION")]
    assert "ss_related_terms" in abi_comment and "SS_MAX_FEEDBACK_DOCS" in abi_comment
    from spaghettisearch_amd import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ss_related_terms")
    assert len(_lib.PROTOTYPES["ss_related_terms"][1]) == 13 and _lib.SS_MAX_FEEDBACK_DOCS == 64
    sig = inspect.signature(engine.Scorer.related_terms)
    assert list(sig.parameters)[1:] == ["q_ptr", "q_terms", "m", "k_fb", "m_doc", "query_len", "topic_probs", "mask_id", "out"]
    assert [sig.parameters[p].default for p in ("m", "k_fb", "m_doc")] == [10, 10, 5]
