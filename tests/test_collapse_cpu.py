"""CPU checks of "collapse by group" (ss_collapse_hits): the sequential model (tests/collapse_model.py) on hand-derived windows with
every expected value written out, the paging identity, and the new entry points in the header, the built library, the ctypes binding
and the engine wrapper (no compute calls — there is no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np

from tests import collapse_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
NO = cm.NO_GROUP

# ten docs: docs 0-3 site 7, docs 4-5 site 0, doc 6 site 0xFFFFFFFE, docs 7-8 never collapsed, doc 9 site 7 again
HAND_GROUP = np.array([7, 7, 7, 7, 0, 0, 0xFFFFFFFE, NO, NO, 7], np.uint32)


def window(docs):
    h = np.zeros((1, len(docs)), cm.HIT_DTYPE)
    h["doc"][0] = docs
    h["_pad"][0] = np.arange(len(docs)) + 100            # every row recognisable, whatever its doc
    h["final"][0] = np.arange(len(docs), dtype=np.float64)   # ascending: NOT the order a scoring call gives
    return h


def run(docs, g, first, k, n=None, fill=0xA5):
    h = window(docs)
    n_hits = np.array([len(docs) if n is None else n], np.int32)
    out = np.frombuffer(bytes([fill]) * (k * 40), cm.HIT_DTYPE).reshape(1, k).copy()
    same = np.full((1, k), 0xA5A5A5A5, np.uint32)
    n_out, n_kept = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    cm.collapse(h, n_hits, HAND_GROUP, g, first, k, out, n_out, same, n_kept)
    return out, int(n_out[0]), same, int(n_kept[0])


def test_hand_derived_window():
    # window rows:    0  1  2  3  4  5  6  7  8   9  10
    docs =           [0, 4, 1, 7, 2, 9, 7, 5, 6, 12, 3]
    # groups:         7  0  7  own 7 7  own 0  FE own(doc >= n_docs) 7
    kept, same = cm.collapse_row(docs, HAND_GROUP, 2)
    assert kept == [0, 1, 2, 3, 6, 7, 8, 9]               # rows 4, 5 and 10 are the third, fourth and fifth of site 7
    assert same == [5, 2, 5, 1, 5, 5, 1, 2, 1, 1, 5]      # over the WHOLE window; the two doc-7 rows are each their own
    kept1, _ = cm.collapse_row(docs, HAND_GROUP, 1)
    assert kept1 == [0, 1, 3, 6, 8, 9]
    kept5, _ = cm.collapse_row(docs, HAND_GROUP, 5)
    assert kept5 == list(range(11))
    out, n_out, same_out, n_kept = run(docs, 2, 2, 4)
    assert (n_out, n_kept) == (4, 8)
    assert out["doc"][0].tolist() == [1, 7, 7, 5] and out["_pad"][0].tolist() == [102, 103, 106, 107]   # window order, whole rows
    assert same_out[0].tolist() == [5, 1, 1, 2]
    # a page that straddles the end: two rows written, the rest untouched
    out, n_out, same_out, n_kept = run(docs, 2, 6, 4)
    assert (n_out, n_kept) == (2, 8) and out["doc"][0, :2].tolist() == [6, 12]
    assert out[0, 2:].tobytes() == b"\xa5" * 80 and same_out[0].tolist() == [1, 1, 0xA5A5A5A5, 0xA5A5A5A5]
    # first at and past the end: nothing written, n_kept still reported
    for first in (8, 9, 1000):
        out, n_out, same_out, n_kept = run(docs, 2, first, 4)
        assert (n_out, n_kept) == (0, 8) and out.tobytes() == b"\xa5" * 160
    # a shorter window: only its rows count, for `same` too
    out, n_out, same_out, n_kept = run(docs, 2, 0, 11, n=5)
    assert (n_out, n_kept) == (4, 4) and out["doc"][0, :4].tolist() == [0, 4, 1, 7] and same_out[0, :4].tolist() == [3, 1, 3, 1]
    out, n_out, _, n_kept = run(docs, 2, 0, 3, n=0)
    assert (n_out, n_kept) == (0, 0) and out.tobytes() == b"\xa5" * 120


def test_same_doc_twice_and_rows_of_their_own():
    # doc 0 twice: one group (site 7), the second row is the site's second; doc 7 twice: two rows of their own, never collapsed
    kept, same = cm.collapse_row([0, 0, 0, 7, 7, 7], HAND_GROUP, 2)
    assert kept == [0, 1, 3, 4, 5] and same == [3, 3, 3, 1, 1, 1]
    # group values at the edges of 32 bits stay apart from each other and from rows of their own
    group = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, NO], np.uint32)
    kept, same = cm.collapse_row([0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 6], group, 1)
    assert kept == [0, 1, 2, 3, 4, 5, 11, 12] and same == [2, 2, 2, 2, 2, 1, 2, 2, 2, 2, 2, 1, 1]


def test_n_hits_outside_the_window():
    h = window([0, 1, 2])
    out, n_out = np.zeros((1, 3), cm.HIT_DTYPE), np.zeros(1, np.int32)
    for bad in (-1, 4):
        try:
            cm.collapse(h, np.array([bad], np.int32), HAND_GROUP, 1, 0, 3, out, n_out)
        except ValueError:
            pass
        else:
            raise AssertionError("host n_hits outside [0, k_in] is an error")
    cm.collapse(h, np.array([-1], np.int32), HAND_GROUP, 1, 0, 3, out, n_out, clamp=True)
    assert n_out[0] == 0
    cm.collapse(h, np.array([8], np.int32), HAND_GROUP, 1, 0, 3, out, n_out, clamp=True)
    assert n_out[0] == 1 and out["doc"][0, 0] == 0


def random_windows(rng, n_q, k_in, n_docs, n_groups):
    group = rng.integers(0, n_groups, n_docs).astype(np.uint32)
    group[rng.random(n_docs) < 0.1] = NO
    h = np.zeros((n_q, k_in), cm.HIT_DTYPE)
    h["doc"] = rng.integers(0, n_docs + 3, (n_q, k_in))
    h["final"] = rng.random((n_q, k_in))
    return h, rng.integers(0, k_in + 1, n_q).astype(np.int32), group


def test_pages_concatenate_to_one_call():
    rng = np.random.default_rng(5)
    h, n_hits, group = random_windows(rng, 40, 37, 60, 6)
    for g in (1, 2, 5):
        whole = np.zeros((40, 37), cm.HIT_DTYPE)
        n_whole, n_kept = np.zeros(40, np.int32), np.zeros(40, np.int32)
        cm.collapse(h, n_hits, group, g, 0, 37, whole, n_whole, None, n_kept)
        assert n_whole.tolist() == n_kept.tolist()
        for k in (1, 4, 36, 37):
            for q in range(40):
                got = []
                for first in range(0, int(n_kept[q]) + k, k):     # one page past the end too: it is empty
                    page, n_page = np.zeros((1, k), cm.HIT_DTYPE), np.zeros(1, np.int32)
                    cm.collapse(h[q:q + 1], n_hits[q:q + 1], group, g, first, k, page, n_page)
                    assert n_page[0] == min(max(int(n_kept[q]) - first, 0), k)
                    got.append(page[0, :n_page[0]].tobytes())
                assert b"".join(got) == whole[q, :n_kept[q]].tobytes(), (g, k, q)


def test_same_sums_to_the_window_length_over_distinct_groups():
    rng = np.random.default_rng(6)
    h, n_hits, group = random_windows(rng, 60, 50, 40, 5)
    for q in range(60):
        docs = h["doc"][q, :n_hits[q]]
        keys = cm.row_groups(docs, group)
        _, same = cm.collapse_row(docs, group, 3)
        first_of = {}
        for j, key in enumerate(keys):
            first_of.setdefault(key, j)
        assert sum(same[j] for j in first_of.values()) == int(n_hits[q])
        kept, _ = cm.collapse_row(docs, group, 10 ** 6)
        assert kept == list(range(int(n_hits[q])))                # g beyond the window: the identity


def test_header_library_binding_and_engine_have_the_calls():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("ss_scorer_set_doc_groups", 2), ("ss_collapse_hits", 12), ("ss_score_topk_collapsed", 15)):
        m = re.search(r"\bint32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
    assert re.search(r"#define SS_NO_GROUP 0xFFFFFFFFu\b", text)
    assert re.search(r"#define SS_ABI_VERSION 4\b", text)
    abi_comment = raw[:raw.index("#define SS_ABI_VERSION")]
    assert all(w in abi_comment for w in ("SS_NO_GROUP", "ss_scorer_set_doc_groups", "ss_collapse_hits", "ss_score_topk_collapsed"))
    from spaghettisearch_amd import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("ss_scorer_set_doc_groups", 2), ("ss_collapse_hits", 12), ("ss_score_topk_collapsed", 15)):
        assert hasattr(lib, name), name
        assert len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert _lib.SS_NO_GROUP == cm.NO_GROUP == 0xFFFFFFFF
    assert ctypes.sizeof(_lib.SsHit) == 40 == engine.HIT_DTYPE.itemsize and engine.HIT_DTYPE == cm.HIT_DTYPE
    assert list(inspect.signature(engine.Scorer.set_doc_groups).parameters)[1:] == ["group"]
    assert list(inspect.signature(engine.Scorer.collapse_hits).parameters)[1:6] == ["hits", "n_hits", "g", "k", "first"]
    assert list(inspect.signature(engine.Scorer.score_topk_collapsed).parameters)[1:7] == ["q_ptr", "q_terms", "k_window", "g", "k", "first"]
