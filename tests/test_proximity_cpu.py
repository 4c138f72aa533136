"""CPU checks of term proximity (ss_hit_proximity, ss_rerank_hits_by_proximity, ss_score_topk_proximity): the numpy model
(tests/proximity_model.py) against an independent brute force over all (a, b) pairs of occurrence values, on random small worlds and
on hand-worked tables with every expected value written out (the header's known answer among them); the re-rank's order on made-up
windows; and the new entry points in the header, the built library, the ctypes binding and the engine wrapper (no compute calls: no
GPU here)."""
import ctypes
import inspect
import os
import re

import numpy as np

from tests import proximity_model as xm
from tests.passage_model import body_lists
from tests.test_passage_cpu import positions_of
from tests.test_related_terms_cpu import table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spaghetti_rank.h")
NAN, INF = float("nan"), float("inf")
UNKNOWN = 0xFFFFFFFF
N_TERMS = 4
ABC = [0, 1, 2]

# One doc per case, in this order; lists: {term: the position list of the term's body posting in that doc}; want: (start, end,
# n_present, n_occ, token_mask).  Term 3 has no posting anywhere.  t: the T of the re-rank's cover.
HAND_CASES = [
    # the header's known answer: docs X, Y, Z, W under the tokens (A, B, C)
    dict(name="X", lists={0: [3.0, 40.0], 1: [5.0, 41.0, 90.0], 2: [43.0, -100.0]}, tokens=ABC, want=(40.0, 43.0, 3, 3, 0b111), t=3),
    dict(name="Y", lists={0: [7.0], 1: [8.0]}, tokens=ABC, want=(7.0, 8.0, 2, 2, 0b011), t=3),
    dict(name="Z", lists={0: [10.0]}, tokens=ABC, want=(10.0, 10.0, 1, 1, 0b001), t=3),
    dict(name="W", lists={}, tokens=ABC, want=(0.0, 0.0, 0, 0, 0), t=3),
    # unsorted lists; two spans of equal difference: the smaller start wins
    dict(name="unsorted", lists={0: [30.0, 2.0, 17.0], 1: [18.0, 1.0]}, tokens=[0, 1], want=(1.0, 2.0, 2, 2, 0b11), t=2),
    # equal values count separately, and the whole run of the end's value lies in the span
    dict(name="equal", lists={0: [5.0, 5.0, 5.0], 1: [5.0, 9.0]}, tokens=[0, 1], want=(5.0, 5.0, 2, 4, 0b11), t=2),
    dict(name="end-run", lists={0: [1.0], 1: [4.0, 4.0], 2: [4.0, 2.0]}, tokens=ABC, want=(1.0, 4.0, 3, 5, 0b111), t=3),
    # both zeros are equal and come back as +0.0
    dict(name="zeros", lists={0: [-0.0], 1: [0.0, -0.0, 3.0]}, tokens=[0, 1], want=(0.0, 0.0, 2, 3, 0b11), t=2),
    # -100, NaN and +inf are no occurrences: term 1 is not present
    dict(name="none-values", lists={0: [NAN, 6.0, INF], 1: [-100.0, INF, NAN]}, tokens=[0, 1], want=(6.0, 6.0, 1, 1, 0b01), t=2),
    dict(name="inf-only", lists={0: [INF], 1: [-100.0]}, tokens=[0, 1], want=(0.0, 0.0, 0, 0, 0), t=2),
    # duplicate tokens: equal bits, one term; T counts ids
    dict(name="dup-tokens", lists={0: [7.0], 1: [8.0]}, tokens=[0, 1, 0], want=(7.0, 8.0, 2, 2, 0b111), t=2),
    # unknown ids (0xFFFFFFFF and the id n_terms) and a term without a posting: each is one id of T
    dict(name="unknown", lists={0: [2.0]}, tokens=[UNKNOWN, N_TERMS, 0, 3, 1], want=(2.0, 2.0, 1, 1, 0b100), t=5),
    dict(name="t-counting", lists={0: [2.0, 9.0]}, tokens=[UNKNOWN, UNKNOWN, 0], want=(2.0, 2.0, 1, 1, 0b100), t=2),
    # |P| = 1: the smallest occurrence alone, with its equals
    dict(name="one-term", lists={0: [9.0, 4.0, 4.0]}, tokens=[0], want=(4.0, 4.0, 1, 2, 0b1), t=1),
    # a term in the middle that pulls the end: A 10 | B 11, 30 | C 12, 31; and a later, tighter span
    dict(name="tighter-later", lists={0: [10.0, 29.5], 1: [13.0, 30.0], 2: [12.0, 30.5]}, tokens=ABC, want=(29.5, 30.5, 3, 3, 0b111), t=3),
    # the difference is the float64 difference of the values: 2^24 + 2 - 2^24 and 3 - 1 tie, the smaller start wins
    dict(name="float64-diff", lists={0: [16777216.0, 1.0], 1: [16777218.0, 3.0]}, tokens=[0, 1], want=(1.0, 3.0, 2, 2, 0b11), t=2),
    # an empty query: nothing present, T = 0
    dict(name="no-tokens", lists={0: [1.0], 1: [2.0]}, tokens=[], want=(0.0, 0.0, 0, 0, 0), t=0),
]
NAMES = [c["name"] for c in HAND_CASES]


def hand_world():
    """-> (n_docs, title, body, body_pos): doc c holds the postings of HAND_CASES[c]; the title table is empty"""
    n_docs = len(HAND_CASES)
    body = table_of([{t: 1.0 for t in c["lists"]} for c in HAND_CASES], N_TERMS)
    title = table_of([{} for _ in HAND_CASES], N_TERMS)
    pos = positions_of([HAND_CASES[d]["lists"][t] for t in range(N_TERMS) for d in range(n_docs) if t in HAND_CASES[d]["lists"]])
    return n_docs, title, body, pos


def entry(e):
    return (float(e["start"]), float(e["end"]), int(e["n_present"]), int(e["n_occ"]), int(e["token_mask"]))


def same(a, b):
    """two (start, end, n_present, n_occ, token_mask): equal as float32 bits and integers"""
    return np.array(a[:2], np.float32).tobytes() == np.array(b[:2], np.float32).tobytes() and tuple(a[2:]) == tuple(b[2:])


def brute(lists, n_terms, n_docs, tokens, d):
    """The definition restated over ALL pairs (a, b): -> (start, end, n_present, n_occ, token_mask) with Python floats and integers.
    lists: {(term, doc): values}."""
    occ = []                                                 # (value, term)
    for t in sorted(set(tokens)):
        if t < n_terms and d < n_docs and (t, d) in lists:
            occ += [(float(v) + 0.0, t) for v in lists[(t, d)] if 0 <= float(v) < INF]
    present = {t for _, t in occ}
    if not present:
        return (0.0, 0.0, 0, 0, 0)
    best = None
    for a, _ in occ:
        for b, _ in occ:
            if a <= b and {t for v, t in occ if a <= v <= b} == present:
                cand = (b - a, a, b)
                if best is None or cand < best:
                    best = cand
    _, a, b = best
    return (a, b, len(present), sum(a <= v <= b for v, _ in occ) & 0xFFFFFFFF, sum(1 << i for i, t in enumerate(tokens) if t in present))


def one_query(tokens):
    return np.array([0, len(tokens)], np.uint32), np.array(tokens, np.uint32)


def test_hand_cases_model_and_brute_force():
    n_docs, title, body, pos = hand_world()
    lists = body_lists(body, pos)
    assert xm.PROXIMITY_DTYPE.itemsize == 24
    for d, c in enumerate(HAND_CASES):
        q_ptr, q_terms = one_query(c["tokens"])
        out = xm.proximity_ref(body, n_docs, q_ptr, q_terms, np.array([[d, 0]], np.uint32), np.array([1], np.int32), body_pos=pos, fill=0xA5)
        assert same(entry(out[0, 0]), c["want"]), (c["name"], entry(out[0, 0]))
        assert same(brute(lists, N_TERMS, n_docs, c["tokens"], d), c["want"]), (c["name"], brute(lists, N_TERMS, n_docs, c["tokens"], d))
        assert out[0, 1].tobytes() == b"\xa5" * 24                            # behind n_hits: untouched
        if c["want"][2] == 0:
            assert out[0, 0].tobytes() == bytes(24)
        assert len(set(c["tokens"])) == c["t"], c["name"]
    # the zeros case: +0.0 bits whichever zeros the lists hold
    z = NAMES.index("zeros")
    out = xm.proximity_ref(body, n_docs, [0, 2], [0, 1], np.array([[z]], np.uint32), [1], body_pos=pos)
    assert out["start"].view(np.uint32)[0, 0] == 0 and out["end"].view(np.uint32)[0, 0] == 0
    # doc >= n_docs, and a body table without positions: zeros, written
    q_ptr, q_terms = one_query([0, 1])
    far = xm.proximity_ref(body, n_docs, q_ptr, q_terms, np.array([[n_docs, UNKNOWN, 0]], np.uint32), [2], body_pos=pos, fill=0xA5)
    assert far[0, :2].tobytes() == bytes(48) and far[0, 2].tobytes() == b"\xa5" * 24
    assert brute(lists, N_TERMS, n_docs, [0, 1], n_docs) == (0.0, 0.0, 0, 0, 0)
    none = xm.proximity_ref(body, n_docs, q_ptr, q_terms, np.array([[0, 1, 7]], np.uint32), [3], body_pos=None, fill=0xA5)
    assert none.tobytes() == bytes(72)


def window_of(docs, finals=None):
    hits = np.zeros((1, len(docs)), dtype=xm.HIT_DTYPE)
    hits["doc"][0] = docs
    if finals is not None:
        hits["final"][0] = finals
    return hits, np.array([len(docs)], np.int32)


def test_known_answer_bonus_and_order():
    n_docs, title, body, pos = hand_world()
    x, y, z, w = (NAMES.index(n) for n in "XYZW")
    q_ptr, q_terms = one_query(ABC)
    ent = xm.proximity_ref(body, n_docs, q_ptr, q_terms, np.array([[x, y, z, w]], np.uint32), [4], body_pos=pos)[0]
    bonus = [xm.bonus_of(e, 3) for e in ent]
    assert bonus[0] == 2.0 / 3.0 * 1.0 and bonus[1] == 1.0 * (2.0 / 3.0) and bonus[0].tobytes() == bonus[1].tobytes()
    assert bonus[2] == 0.0 and bonus[3] == 0.0
    hits, n_hits = window_of([w, z, y, x], [0.9, 0.8, 0.7, 0.6])
    o_hits, o_n, o_sc, o_px = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 0.0, 1.0, 0, 4, body_pos=pos, fill=0xA5)
    assert o_hits["doc"][0].tolist() == [y, x, w, z] and o_n.tolist() == [4]
    assert o_sc[0].tolist() == [2.0 / 3.0, 2.0 / 3.0, 0.0, 0.0]
    assert [entry(e) for e in o_px[0]] == [HAND_CASES[d]["want"] for d in (y, x, w, z)]
    # w_prox == 0, w_rank > 0 on rows in FinalRank order: the window, its inside rows first
    hits, n_hits = window_of([w, n_docs + 1, z, y, UNKNOWN, x], [0.9, 0.85, 0.8, 0.7, 0.65, 0.6])
    o_hits, o_n, o_sc, o_px = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 2.0, 0.0, 0, 6, body_pos=pos, fill=0xA5)
    assert o_hits["doc"][0].tolist() == [w, z, y, x, n_docs + 1, UNKNOWN]
    assert o_sc.view(np.uint64)[0, 4:].tolist() == [xm.NAN_BITS] * 2 and o_px[0, 4:].tobytes() == bytes(48)
    # paging, NaN finals behind every number, -0.0 ties 0.0, the same doc twice is two rows
    # (every bonus is 0.0 here and w_prox * bonus = -0.0, so the score is the final with its sign of zero)
    hits, n_hits = window_of([z, z, w, w, z], [-0.0, NAN, 0.0, -1.0, INF])
    o_hits, o_n, o_sc, _ = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 1.0, -1.0, 0, 5, body_pos=pos, fill=0xA5)
    assert o_hits["final"].view(np.uint64)[0].tolist() == hits["final"].view(np.uint64)[0, [4, 0, 2, 3, 1]].tolist()
    assert o_sc.view(np.uint64)[0].tolist() == [0x7FF0000000000000, 0x8000000000000000, 0, 0xBFF0000000000000, xm.NAN_BITS]
    o_hits, o_n, o_sc, _ = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 1.0, -1.0, 3, 4, body_pos=pos, fill=0xA5)
    assert o_n.tolist() == [2] and o_hits[0, 2:].tobytes() == b"\xa5" * 80 and o_sc[0, 2:].tobytes() == b"\xa5" * 16
    assert xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 1.0, -1.0, 5, 4, body_pos=pos)[1].tolist() == [0]
    # an empty query: T = 0, cover 0, every bonus 0: window order
    e_ptr, e_terms = one_query([])
    o_hits, _, o_sc, _ = xm.rerank_ref(body, n_docs, e_ptr, e_terms, *window_of([x, y, z], [1.0, 1.0, 1.0]), 0.0, 1.0, 0, 3, body_pos=pos)
    assert o_hits["doc"][0].tolist() == [x, y, z] and o_sc[0].tolist() == [0.0, 0.0, 0.0]


def random_world(seed):
    """a small world whose lists collide often: 12 docs, 5 terms, values from a handful of numbers, -100 / NaN / +inf / -0.0 mixed in"""
    rng = np.random.default_rng(seed)
    n_docs, n_terms = 12, 5
    rows = [{t: 1.0 for t in range(n_terms) if rng.random() < 0.6} for _ in range(n_docs)]
    body = table_of(rows, n_terms)
    pool = np.array([0.0, -0.0, 1.0, 2.0, 2.5, 3.0, 7.0, 8.0, 20.0, 21.0, 500.0, -100.0, NAN, INF])
    lists = [rng.choice(pool, size=int(rng.integers(0, 7))).tolist() for _ in range(len(body[1]))]
    return n_docs, n_terms, body, positions_of(lists)


def test_model_equals_brute_force_on_random_small_worlds():
    seen = {"multi": 0, "none": 0, "tie": 0}
    for seed in range(12):
        n_docs, n_terms, body, pos = random_world(seed)
        lists = body_lists(body, pos)
        rng = np.random.default_rng(100 + seed)
        rows = [rng.integers(0, n_terms + 2, size=int(n)).tolist() for n in (1, 2, 3, 3, 5, 0)] + [[UNKNOWN, 1, 1, 0]]
        q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
        q_terms = np.array([t for r in rows for t in r], np.uint32)
        docs = np.tile(np.arange(n_docs + 1, dtype=np.uint32), (len(rows), 1))
        n_hits = np.full(len(rows), n_docs + 1, np.int32)
        out = xm.proximity_ref(body, n_docs, q_ptr, q_terms, docs, n_hits, body_pos=pos, fill=0xA5)
        for q, toks in enumerate(rows):
            for d in range(n_docs + 1):
                want = brute(lists, n_terms, n_docs, toks, d)
                assert same(entry(out[q, d]), want), (seed, q, d, entry(out[q, d]), want)
                seen["multi"] += want[2] > 1
                seen["none"] += want[2] == 0
    assert seen["multi"] > 100 and seen["none"] > 100, seen


def test_rerank_consequences_on_a_random_world():
    n_docs, n_terms, body, pos = random_world(3)
    rows = [[0, 1, 2], [3, 4], [1, 1, UNKNOWN, 2]]
    q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    q_terms = np.array([t for r in rows for t in r], np.uint32)
    rng = np.random.default_rng(5)
    k_in = 14
    hits = np.zeros((3, k_in), dtype=xm.HIT_DTYPE)
    hits["doc"] = rng.integers(0, n_docs + 2, size=(3, k_in))
    hits["final"] = -np.sort(-rng.random((3, k_in)), axis=1)
    n_hits = np.array([k_in, 9, 0], np.int32)
    # w_rank == 0: bonus descending, then window order
    o_hits, o_n, o_sc, o_px = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 0.0, 3.0, 0, k_in, body_pos=pos, fill=0xA5)
    assert o_n.tolist() == [k_in, 9, 0] and o_hits[2].tobytes() == b"\xa5" * (k_in * 40)
    for q in range(2):
        n = int(n_hits[q])
        inside = [j for j in range(n) if hits["doc"][q, j] < n_docs]
        ent = xm.proximity_ref(body, n_docs, q_ptr, q_terms, hits["doc"], n_hits, body_pos=pos)
        bonus = {j: float(xm.bonus_of(ent[q, j], len(set(rows[q])))) for j in inside}
        order = sorted(inside, key=lambda j: (-bonus[j], j)) + [j for j in range(n) if j not in inside]
        assert o_hits[q, :n].tobytes() == hits[q, order].tobytes()
        assert o_sc[q, :len(inside)].tolist() == [3.0 * bonus[j] for j in order[:len(inside)]]
    # w_prox == 0, w_rank > 0: the window with its inside rows first
    o_hits, o_n, _, _ = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 0.5, 0.0, 0, k_in, body_pos=pos)
    for q in range(2):
        n = int(n_hits[q])
        order = [j for j in range(n) if hits["doc"][q, j] < n_docs] + [j for j in range(n) if hits["doc"][q, j] >= n_docs]
        assert o_hits[q, :n].tobytes() == hits[q, order].tobytes()
    # the scored form is the re-rank of the rows it is given
    a = xm.score_topk_proximity_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 1.0, 0.25, 2, 5, body_pos=pos, fill=0xA5)
    b = xm.rerank_ref(body, n_docs, q_ptr, q_terms, hits, n_hits, 1.0, 0.25, 2, 5, body_pos=pos, fill=0xA5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def prototype(text, name):
    m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text, flags=re.S)
    return m and [a.strip() for a in m.group(1).split(",")]


def test_header_library_binding_and_engine_have_the_calls():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    counts = {"ss_hit_proximity": 8, "ss_rerank_hits_by_proximity": 15, "ss_score_topk_proximity": 16}
    for name, n_args in counts.items():
        args = prototype(text, name)
        assert args and len(args) == n_args, (name, args)
    assert [a for a in prototype(text, "ss_rerank_hits_by_proximity") if a.startswith("double ")] == ["double w_rank", "double w_prox"]
    s = re.search(r"typedef\s+struct\s+ss_proximity\s*\{([^}]*)\}\s*ss_proximity\s*;", text)
    assert s and re.findall(r"(\w+)\s+(\w+)\s*;", s.group(1)) == [("float", "start"), ("float", "end"), ("uint32_t", "n_present"),
                                                                 ("uint32_t", "n_occ"), ("uint64_t", "token_mask")]
    assert re.search(r"#define SS_ABI_VERSION 4\b", text)
    abi_comment = raw[:raw.index("#define SS_ABI_VERSION")]
    assert all(n in abi_comment for n in list(counts) + ["ss_proximity"])
    from spaghettisearch_amd import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in counts.items():
        assert hasattr(lib, name), name
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    assert _lib.PROTOTYPES["ss_rerank_hits_by_proximity"][1][7:9] == [ctypes.c_double, ctypes.c_double]
    assert _lib.PROTOTYPES["ss_score_topk_proximity"][1][8:10] == [ctypes.c_double, ctypes.c_double]
    assert ctypes.sizeof(_lib.SsProximity) == 24 == engine.PROXIMITY_DTYPE.itemsize == xm.PROXIMITY_DTYPE.itemsize
    assert engine.PROXIMITY_DTYPE == xm.PROXIMITY_DTYPE and engine.HIT_DTYPE == xm.HIT_DTYPE
    offsets = {"start": 0, "end": 4, "n_present": 8, "n_occ": 12, "token_mask": 16}
    assert {n: engine.PROXIMITY_DTYPE.fields[n][1] for n in engine.PROXIMITY_DTYPE.names} == offsets
    assert {n: getattr(_lib.SsProximity, n).offset for n in offsets} == offsets
    sig = inspect.signature(engine.Scorer.hit_proximity)
    assert list(sig.parameters)[1:7] == ["q_ptr", "q_terms", "hits", "n_hits", "out", "k"]
    sig = inspect.signature(engine.Scorer.rerank_by_proximity)
    assert list(sig.parameters)[1:11] == ["q_ptr", "q_terms", "hits", "n_hits", "k", "w_rank", "w_prox", "first", "k_in", "out"]
    sig = inspect.signature(engine.Scorer.score_topk_proximity)
    assert list(sig.parameters)[1:8] == ["q_ptr", "q_terms", "k_window", "k", "w_rank", "w_prox", "first"]
