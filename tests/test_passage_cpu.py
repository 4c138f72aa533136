"""CPU checks of "best passage per hit" (ss_best_passages): the numpy model (tests/passage_model.py) against an independent
brute-force restatement of the header's definition (every occurrence as a start, every window by a loop, integers and Python
floats), on hand-worked tables with every expected value written out and on the golden 300 x 80 tables with random positions; and
the new entry point in the header, the built library, the ctypes binding and the engine wrapper (no compute calls: no GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np

from tests import passage_model as pm
from tests.test_related_terms_cpu import table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "index_300x80.npz")
NAN = float("nan")
UNKNOWN = 0xFFFFFFFF
N_TERMS = 4

# One doc per case, in this order; lists: {term: the position list of the term's body posting in that doc}; want: (start, last,
# n_distinct, n_occ, token_mask).  Term 3 has no posting anywhere.
HAND_CASES = [
    # two windows tied on both counts: the earliest wins
    dict(name="tie", lists={0: [1.0, 50.0], 1: [2.0, 51.0]}, tokens=[0, 1], width=5, want=(1.0, 2.0, 2, 2, 0b11)),
    # more distinct terms beats more occurrences
    dict(name="distinct", lists={0: [10.0, 11.0, 12.0, 13.0, 99.0], 1: [100.0]}, tokens=[0, 1], width=5, want=(99.0, 100.0, 2, 2, 0b11)),
    # a value exactly at p + width is excluded, one below it is not
    dict(name="limit", lists={0: [3.0], 1: [8.0]}, tokens=[0, 1], width=5, want=(3.0, 3.0, 1, 1, 0b01)),
    dict(name="below-limit", lists={0: [3.0], 1: [8.0]}, tokens=[0, 1], width=6, want=(3.0, 8.0, 2, 2, 0b11)),
    # width 1: [4, 5) holds 4 and 4.5, [4.5, 5.5) holds 4.5 and 5
    dict(name="width-1", lists={0: [4.0, 4.5], 1: [5.0]}, tokens=[0, 1], width=1, want=(4.5, 5.0, 2, 2, 0b11)),
    # duplicate tokens: equal bits, one distinct term
    dict(name="dup-tokens", lists={0: [7.0], 1: [8.0]}, tokens=[0, 1, 0], width=5, want=(7.0, 8.0, 2, 2, 0b111)),
    # duplicate values count separately
    dict(name="dup-values", lists={0: [5.0, 5.0, 5.0], 1: [9.0]}, tokens=[0, 1], width=3, want=(5.0, 5.0, 1, 3, 0b01)),
    # unsorted lists
    dict(name="unsorted", lists={0: [30.0, 2.0, 17.0], 1: [18.0, 1.0]}, tokens=[0, 1], width=3, want=(1.0, 2.0, 2, 2, 0b11)),
    # both zeros are equal and come back as +0.0
    dict(name="zeros", lists={0: [-0.0], 1: [0.0, -0.0]}, tokens=[0, 1], width=1, want=(0.0, 0.0, 2, 3, 0b11)),
    # NaN and -100 are no occurrences
    dict(name="nan", lists={0: [NAN, 6.0], 1: [NAN]}, tokens=[0, 1], width=5, want=(6.0, 6.0, 1, 1, 0b01)),
    dict(name="marker", lists={0: [-100.0, -100.0], 1: [-100.0, 3.0]}, tokens=[0, 1], width=5, want=(3.0, 3.0, 1, 1, 0b10)),
    # unknown terms (0xFFFFFFFF and the id n_terms) and a term without a posting in the doc
    dict(name="unknown", lists={0: [2.0]}, tokens=[UNKNOWN, N_TERMS, 0, 3, 1], width=5, want=(2.0, 2.0, 1, 1, 0b100)),
    # nothing but markers; a missing posting; a query without tokens: 24 zero bytes
    dict(name="no-occurrence", lists={0: [-100.0], 1: []}, tokens=[0, 1], width=5, want=(0.0, 0.0, 0, 0, 0)),
    dict(name="no-posting", lists={0: [1.0]}, tokens=[1, 3], width=5, want=(0.0, 0.0, 0, 0, 0)),
    dict(name="no-tokens", lists={0: [1.0], 1: [2.0]}, tokens=[], width=5, want=(0.0, 0.0, 0, 0, 0)),
]


def positions_of(lists):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    return ptr, np.array([v for x in lists for v in x], dtype=np.float32)


def hand_world():
    """-> (n_docs, title, body, body_pos): doc c holds the postings of HAND_CASES[c]; the title table is empty"""
    n_docs = len(HAND_CASES)
    body = table_of([{t: 1.0 for t in c["lists"]} for c in HAND_CASES], N_TERMS)
    title = table_of([{} for _ in HAND_CASES], N_TERMS)
    pos = positions_of([HAND_CASES[d]["lists"][t] for t in range(N_TERMS) for d in range(n_docs) if t in HAND_CASES[d]["lists"]])
    return n_docs, title, body, pos


def random_positions(n_post, seed, long_every=0):
    """unsorted lists of 0 - 6 positions with -100 markers mixed in; every long_every-th list holds 70 - 200 values"""
    rng = np.random.default_rng(seed)
    lists = []
    for x in range(n_post):
        n = int(rng.integers(70, 201)) if long_every and x % long_every == 0 else int(rng.integers(0, 7))
        vals = rng.integers(0, 5000, size=n).astype(float)
        vals[rng.random(n) < 0.2] = -100.0
        lists.append(vals.tolist())
    return positions_of(lists)


def entry(e):
    return (float(e["start"]), float(e["last"]), int(e["n_distinct"]), int(e["n_occ"]), int(e["token_mask"]))


def brute(lists, n_terms, n_docs, tokens, d, width):
    """The definition restated: -> (start, last, n_distinct, n_occ, token_mask) with Python floats and integers.  lists: {(term, doc):
    values}."""
    occ = []                                                 # (value, term)
    for t in sorted(set(tokens)):
        if t < n_terms and d < n_docs and (t, d) in lists:
            occ += [(float(v), t) for v in lists[(t, d)] if float(v) >= 0]
    best = None
    for p, _ in occ:
        inside = [(v, t) for v, t in occ if v >= p and v < p + float(width)]
        if not inside:
            continue
        terms = {t for _, t in inside}
        cand = (len(terms), len(inside), -p)
        if best is None or cand > best[0]:
            best = (cand, max(v for v, _ in inside), terms)
    if best is None:
        return (0.0, 0.0, 0, 0, 0)
    (nd, nocc, neg_p), last, terms = best
    return (-neg_p + 0.0, last + 0.0, nd, nocc & 0xFFFFFFFF, sum(1 << i for i, t in enumerate(tokens) if t in terms))


def same(a, b):
    """two (start, last, n_distinct, n_occ, token_mask): equal as float32 bits and integers"""
    return np.array(a[:2], np.float32).tobytes() == np.array(b[:2], np.float32).tobytes() and tuple(a[2:]) == tuple(b[2:])


def test_hand_cases_model_and_brute_force():
    n_docs, title, body, pos = hand_world()
    lists = pm.body_lists(body, pos)
    assert pm.PASSAGE_DTYPE.itemsize == 24
    for d, c in enumerate(HAND_CASES):
        q_ptr, q_terms = np.array([0, len(c["tokens"])], np.uint32), np.array(c["tokens"], np.uint32)
        out = pm.passages_ref(body, n_docs, q_ptr, q_terms, np.array([[d, 0]], np.uint32), np.array([1], np.int32), c["width"], body_pos=pos,
                              fill=0xA5)
        assert same(entry(out[0, 0]), c["want"]), (c["name"], entry(out[0, 0]))
        assert same(brute(lists, N_TERMS, n_docs, c["tokens"], d, c["width"]), c["want"]), c["name"]
        assert out[0, 1].tobytes() == b"\xa5" * 24                            # behind n_hits: untouched
        if c["want"][3] == 0:
            assert out[0, 0].tobytes() == bytes(24)
    # the zeros case: +0.0 bits whichever zeros the lists hold
    z = [c["name"] for c in HAND_CASES].index("zeros")
    out = pm.passages_ref(body, n_docs, [0, 2], [0, 1], np.array([[z]], np.uint32), [1], 1, body_pos=pos)
    assert out["start"].view(np.uint32)[0, 0] == 0 and out["last"].view(np.uint32)[0, 0] == 0
    # doc >= n_docs, and a body table without positions: zeros, written
    q_ptr, q_terms = np.array([0, 2], np.uint32), np.array([0, 1], np.uint32)
    far = pm.passages_ref(body, n_docs, q_ptr, q_terms, np.array([[n_docs, UNKNOWN, 0]], np.uint32), [2], 5, body_pos=pos, fill=0xA5)
    assert far[0, :2].tobytes() == bytes(48) and far[0, 2].tobytes() == b"\xa5" * 24
    assert brute(lists, N_TERMS, n_docs, [0, 1], n_docs, 5) == (0.0, 0.0, 0, 0, 0)
    none = pm.passages_ref(body, n_docs, q_ptr, q_terms, np.array([[0, 1, 7]], np.uint32), [3], 5, body_pos=None, fill=0xA5)
    assert none.tobytes() == bytes(72)
    # an infinite position is an occurrence whose own window is empty
    inf = pm.best_window(np.array([np.inf], np.float32), np.array([0]), [0], 5)
    assert inf.tobytes() == bytes(24)
    both = pm.best_window(np.array([3.0, np.inf], np.float32), np.array([0, 1]), [0, 1], 1 << 24)
    assert entry(both) == (3.0, 3.0, 1, 1, 0b01)


def golden_world():
    z = np.load(GOLDEN)
    body = (z["b_ptr"], z["b_doc"], z["b_w"])
    return int(z["n_docs"]), len(z["b_ptr"]) - 1, body, random_positions(len(z["b_doc"]), 8, long_every=9)


def test_model_equals_brute_force_on_the_golden_tables():
    n_docs, n_terms, body, pos = golden_world()
    lists = pm.body_lists(body, pos)
    rows = [[3], [0, 1, 2], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [UNKNOWN, n_terms], [70, 5, 70], [79, 40, UNKNOWN, 1, 1, n_terms, 33, 2, 60]]
    q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    q_terms = np.array([t for r in rows for t in r], np.uint32)
    rng = np.random.default_rng(21)
    k = 10
    hits_doc = rng.integers(0, n_docs, size=(len(rows), k)).astype(np.uint32)
    for q, toks in enumerate(rows):                          # the first six hits hold the query's first known term
        t = next((t for t in toks if t < n_terms), None)
        if t is not None:
            hits_doc[q, :6] = rng.choice(body[1][int(body[0][t]):int(body[0][t + 1])], 6, replace=False)
    hits_doc[:, -1] = n_docs + 3
    n_hits = np.array([k, k, k, k, k - 2, k], np.int32)
    seen = {"multi": 0, "none": 0}
    for width in (1, 5, 20, 6000):
        out = pm.passages_ref(body, n_docs, q_ptr, q_terms, hits_doc, n_hits, width, body_pos=pos, fill=0xA5)
        for q, toks in enumerate(rows):
            for j in range(k):
                if j >= n_hits[q]:
                    assert out[q, j].tobytes() == b"\xa5" * 24
                    continue
                want = brute(lists, n_terms, n_docs, toks, int(hits_doc[q, j]), width)
                assert same(entry(out[q, j]), want), (width, q, j, entry(out[q, j]), want)
                seen["multi"] += want[2] > 1
                seen["none"] += want[3] == 0
    assert seen["multi"] > 10 and seen["none"] > 10, seen


def test_header_library_binding_and_engine_have_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint32_t\s+ss_best_passages\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == 9
    s = re.search(r"typedef\s+struct\s+ss_passage\s*\{([^}]*)\}\s*ss_passage\s*;", text)
    assert s and re.findall(r"(\w+)\s+(\w+)\s*;", s.group(1)) == [("float", "start"), ("float", "last"), ("uint32_t", "n_distinct"),
                                                                 ("uint32_t", "n_occ"), ("uint64_t", "token_mask")]
    assert re.search(r"#define SS_ABI_VERSION 4\b", text)
    abi_comment = raw[:raw.index("#define SS_ABI_VERSION")]
    assert "ss_best_passages" in abi_comment and "ss_passage" in abi_comment
    from spaghettisearch_amd import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ss_best_passages")
    assert len(_lib.PROTOTYPES["ss_best_passages"][1]) == 9
    assert ctypes.sizeof(_lib.SsPassage) == 24 == engine.PASSAGE_DTYPE.itemsize == pm.PASSAGE_DTYPE.itemsize
    assert engine.PASSAGE_DTYPE == pm.PASSAGE_DTYPE
    offsets = {"start": 0, "last": 4, "n_distinct": 8, "n_occ": 12, "token_mask": 16}
    assert {n: engine.PASSAGE_DTYPE.fields[n][1] for n in engine.PASSAGE_DTYPE.names} == offsets
    assert {n: getattr(_lib.SsPassage, n).offset for n in offsets} == offsets
    sig = inspect.signature(engine.Scorer.best_passages)
    assert list(sig.parameters)[1:8] == ["q_ptr", "q_terms", "hits", "n_hits", "width", "out", "k"]
    assert sig.parameters["out"].default is None and sig.parameters["k"].default is None
