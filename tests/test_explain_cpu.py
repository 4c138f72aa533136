"""CPU checks of "explain hits" (ss_explain_hits): the numpy model (tests/explain_model.py) on hand-worked tables with every
expected value written out, and the new entry point in the header, the built library, the ctypes binding and the engine wrapper
(no compute calls — there is no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np

from tests import explain_model as xm
from tests.test_related_terms_cpu import table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
F32 = np.float32
NAN = float("nan")

# five docs, four terms.  title: term 0 in docs 0 and 2, term 1 in doc 1.  body: term 0 in docs 1 and 2, term 2 in docs 0, 1, 2, 3.
# Term 3 has no posting at all; doc 4 has none either.
HAND_TITLE = [{0: 1.5}, {1: 2.5}, {0: 0.25}, {}, {}]
HAND_BODY = [{2: 3.0}, {0: 0.5, 2: 4.0}, {0: 0.75, 2: 5.0}, {2: 6.0}, {}]
# the body postings in table order: term 0: (doc 1, doc 2)   term 2: (doc 0, doc 1, doc 2, doc 3)
HAND_POS = [[7.0, 2.0], [], [-100.0], [NAN, 7.0, 3.0], [-100.0, 0.0], [4.0]]
UNKNOWN = 0xFFFFFFFF


def positions_of(lists):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    return ptr, np.array([v for x in lists for v in x], dtype=np.float32)


def entry(e):
    """(title_w, body_w, flags, body_pos) of one entry as Python values"""
    return (float(e["title_w"]), float(e["body_w"]), int(e["flags"]), float(e["body_pos"]))


def test_earliest_position_lists():
    assert xm.earliest_position([]) is None
    assert xm.earliest_position([-100.0]) is None
    assert xm.earliest_position([NAN, 7.0, 3.0]) == 3.0
    assert xm.earliest_position([-100.0, 0.0]) == 0.0
    assert xm.earliest_position([NAN, NAN]) is None
    assert xm.earliest_position([5.0, float("inf"), 2.5, -1.0]) == 2.5
    assert xm.earliest_position([float("inf")]) == float("inf")
    # a smallest value of zero is +0.0 whichever zeros the list holds
    for zeros in ([-0.0], [0.0, -0.0], [-0.0, 0.0], [3.0, -0.0]):
        z = xm.earliest_position(zeros)
        assert z == 0.0 and not np.signbit(z) and z.dtype == np.float32, zeros


def test_hand_worked_entries():
    title, body = table_of(HAND_TITLE, 4), table_of(HAND_BODY, 4)
    assert body[0].tolist() == [0, 2, 2, 6, 6] and body[1].tolist() == [1, 2, 0, 1, 2, 3]
    pos = positions_of(HAND_POS)
    # query 0: tokens (0, 2, UNKNOWN, 0) over the hits docs 2, 0, 4;  query 1: token (3) over doc 1;  query 2: no tokens, one hit;
    # query 3: tokens (1, 2) and no hits
    q_ptr = np.array([0, 4, 5, 5, 7], np.uint32)
    q_terms = np.array([0, 2, UNKNOWN, 0, 3, 1, 2], np.uint32)
    hits_doc = np.array([[2, 0, 4], [1, 9, 9], [0, 9, 9], [9, 9, 9]], np.uint32)
    n_hits = np.array([3, 1, 1, 0], np.int32)
    out = xm.explain_ref(title, body, 5, q_ptr, q_terms, hits_doc, n_hits, 4, body_pos=pos, fill=0xA5)
    assert out.dtype == xm.TERM_MATCH_DTYPE and out.shape == (4, 3, 4) and out.dtype.itemsize == 16
    # doc 2: term 0 in both tables (body list [] -> no position), term 2 in the body only with the list [-100, 0]
    assert entry(out[0, 0, 0]) == (0.25, 0.75, 3, 0.0)
    assert entry(out[0, 0, 1]) == (0.0, 5.0, 2 | 4, 0.0)
    assert entry(out[0, 0, 2]) == (0.0, 0.0, 0, 0.0)                      # the unknown term
    assert out[0, 0, 3].tobytes() == out[0, 0, 0].tobytes()               # the duplicate token: the same entry
    # doc 0: term 0 in the title only, term 2 in the body only with the list [-100]: no position
    assert entry(out[0, 1, 0]) == (1.5, 0.0, 1, 0.0)
    assert entry(out[0, 1, 1]) == (0.0, 3.0, 2, 0.0)
    assert entry(out[0, 1, 2]) == (0.0, 0.0, 0, 0.0) and out[0, 1, 3].tobytes() == out[0, 1, 0].tobytes()
    # doc 4: neither table
    assert all(entry(out[0, 2, i]) == (0.0, 0.0, 0, 0.0) for i in range(4))
    # query 1: term 3 has no postings: written, all zero; its slots behind the first token and the first hit are untouched
    assert entry(out[1, 0, 0]) == (0.0, 0.0, 0, 0.0)
    untouched = b"\xa5" * 16
    assert all(out[1, 0, i].tobytes() == untouched for i in (1, 2, 3))
    assert all(out[1, j, i].tobytes() == untouched for j in (1, 2) for i in range(4))
    # query 2 (no tokens) and query 3 (no hits): nothing is written
    assert out[2].tobytes() == untouched * 12 and out[3].tobytes() == untouched * 12
    # the other hits of the position lists: doc 1 holds term 0 with [7, 2] and term 2 with [NaN, 7, 3]; doc 3 term 2 with [4]
    q_ptr2, q_terms2 = np.array([0, 2], np.uint32), np.array([0, 2], np.uint32)
    out2 = xm.explain_ref(title, body, 5, q_ptr2, q_terms2, np.array([[1, 3]], np.uint32), np.array([2], np.int32), 2, body_pos=pos)
    assert entry(out2[0, 0, 0]) == (0.0, 0.5, 2 | 4, 2.0)
    assert entry(out2[0, 0, 1]) == (0.0, 4.0, 2 | 4, 3.0)
    assert entry(out2[0, 1, 0]) == (0.0, 0.0, 0, 0.0)
    assert entry(out2[0, 1, 1]) == (0.0, 6.0, 2 | 4, 4.0)
    # without positional postings bit 2 is never set
    out3 = xm.explain_ref(title, body, 5, q_ptr2, q_terms2, np.array([[1, 3]], np.uint32), np.array([2], np.int32), 2)
    assert [entry(e) for e in out3[0].reshape(-1)] == [(0.0, 0.5, 2, 0.0), (0.0, 4.0, 2, 0.0), (0.0, 0.0, 0, 0.0), (0.0, 6.0, 2, 0.0)]


def test_made_up_hits_and_stored_bits():
    """a doc id at or past n_docs has no postings; a stored -0.0 / NaN weight comes back as it is with its flag set"""
    title = table_of([{0: F32(-0.0)}, {0: F32(NAN)}, {0: F32(0.0)}], 1)
    body = table_of([{}, {}, {}], 1)
    q_ptr, q_terms = np.array([0, 1], np.uint32), np.array([0], np.uint32)
    out = xm.explain_ref(title, body, 3, q_ptr, q_terms, np.array([[0, 1, 2, 3, 0xFFFFFFFF]], np.uint32), np.array([5], np.int32), 1)
    assert out["flags"][0, :, 0].tolist() == [1, 1, 1, 0, 0]
    assert out["title_w"][0, :, 0].tobytes() == np.array([-0.0, NAN, 0.0, 0.0, 0.0], np.float32).tobytes()
    assert out[0, 3:].tobytes() == bytes(32)


def test_header_library_binding_and_engine_have_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint32_t\s+ss_explain_hits\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == 9
    s = re.search(r"typedef\s+struct\s+ss_term_match\s*\{([^}]*)\}\s*ss_term_match\s*;", text)
    assert s and re.findall(r"(\w+)\s+(\w+)\s*;", s.group(1)) == [("float", "title_w"), ("float", "body_w"), ("uint32_t", "flags"),
                                                                 ("float", "body_pos")]
    assert re.search(r"#define SS_ABI_VERSION 4\b", text)
    abi_comment = raw[:raw.index("#define SS_ABI_VERSION")]
    assert "ss_explain_hits" in abi_comment and "ss_term_match" in abi_comment
    from spaghettisearch_amd import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ss_explain_hits")
    assert len(_lib.PROTOTYPES["ss_explain_hits"][1]) == 9
    assert ctypes.sizeof(_lib.SsTermMatch) == 16 == engine.TERM_MATCH_DTYPE.itemsize == xm.TERM_MATCH_DTYPE.itemsize
    assert engine.TERM_MATCH_DTYPE == xm.TERM_MATCH_DTYPE
    sig = inspect.signature(engine.Scorer.explain_hits)
    assert list(sig.parameters)[1:7] == ["q_ptr", "q_terms", "hits", "n_hits", "t_stride", "out"]
    assert sig.parameters["t_stride"].default is None and sig.parameters["out"].default is None
