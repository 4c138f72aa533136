"""GPU parity: ss_facet_counts vs the set model of the header's definition (tests/facet_model.py) and vs the n_hits of
ss_score_topk_filtered.  The tables are synthetic: one full doc block of k_facet_counts plus a partial one whose last word is partial
too, the smallest shape with a block seam, a word seam and the d < n_docs cut.  Every count equals the model's exactly; outputs start
from 0xA5 bytes, so an entry the call must not write is checked with the ones it must."""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import facet_model as fm
from tests.test_gpu_query_constraints import pack_pairs
from tests.test_gpu_score import close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
FILL = 0xA5
BLOCK = 32768                    # docs of one k_facet_counts workgroup: BLOCK_DOCS in csrc/facet_plan.hpp (test_facet_cpu.py drives it)
N_DOCS = BLOCK + 37
N_TERMS = 37
MAX_TOPK, MAX_BUCKETS = 1024, 64
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
UNKNOWN = 0xFFFFFFFF
LAST = N_DOCS - 1
# terms 7 .. 24 have a list in both tables (18 terms, 36 lists), 25 .. 30 a body list only; 31 .. 36 are long
BOTH = list(range(7, 25))


def filled(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytes([FILL]) * n, dtype=dtype).reshape(shape).copy()


def make_world():
    rng = np.random.default_rng(2024)
    title = {0: [3, 100, BLOCK - 1, BLOCK], 2: [7, 100, 300]}
    body = {1: [0, 100, 200, LAST], 2: [7, 300, 500, BLOCK + 2], 3: [900, 901], 4: [BLOCK + 1, BLOCK + 32], 5: [10, 20]}    # 6: no posting at all
    for t in range(7, 31):
        docs = rng.choice(N_DOCS, int(rng.integers(30, 56)), replace=False)
        docs[:4] = [BLOCK - 1 - t, BLOCK + t, 31 + t % 3, LAST - t % 5]        # both blocks, a word seam, the last word
        body[t] = sorted(set(docs.tolist()))
        if t in BOTH:
            title[t] = sorted(set(rng.choice(body[t], 6, replace=False).tolist() + rng.choice(N_DOCS, 6, replace=False).tolist()))
    for t in range(31, N_TERMS):
        body[t] = np.nonzero(rng.random(N_DOCS) < 0.05 * (t - 30))[0].tolist()
        title[t] = np.nonzero(rng.random(N_DOCS) < 0.01)[0].tolist()

    def table(lists):
        ptr = np.zeros(N_TERMS + 1, dtype=np.uint64)
        docs = []
        for t in range(N_TERMS):
            docs += lists.get(t, [])
            ptr[t + 1] = len(docs)
        w = rng.random(len(docs)).astype(np.float32) + np.float32(0.25)
        return ptr, np.array(docs, dtype=np.uint32), w

    title, body = table(title), table(body)
    body[2][int(body[0][3])] = 0.0                                              # term 3's posting on doc 900 has weight zero: it counts
    edge = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64)
    values = np.stack([rng.integers(0, 1000, N_DOCS), edge[rng.integers(0, len(edge), N_DOCS)],
                       (rng.lognormal(9.0, 1.5, N_DOCS)).astype(np.int64)]).astype(np.int64)
    masks = rng.random((3, N_DOCS)) < np.array([0.5, 0.05, 0.9])[:, None]
    masks[1, [100, BLOCK - 1, BLOCK, LAST]] = True
    words = engine.pack_doc_masks(masks, N_DOCS)
    words[2, -1] |= np.uint32(0xFFFFFFFF << (N_DOCS % 32) & 0xFFFFFFFF)         # garbage bits past n_docs: ignored
    return {"title": title, "body": body, "values": values, "masks": masks, "words": words}


@pytest.fixture(scope="module")
def world():
    return make_world()


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, N_DOCS, world["title"], world["body"], np.ones(N_DOCS), np.ones(N_DOCS))
    sc.set_doc_fields(world["values"])
    sc.set_doc_masks(world["words"])
    yield sc
    close_all(sc, ti, bi)


def model(world, queries, n_masks=3, mask_id=None, req=None, exc=None, clauses=None, buckets=()):
    q_ptr, q_terms = pack_pairs(queries)
    masks = fm.unpack_masks(world["words"][:n_masks], N_DOCS)
    ranges = None if clauses is None else (engine.pack_doc_ranges(clauses)[0], [c for cs in clauses for c in cs])
    return fm.facet_counts(N_DOCS, world["title"][:2], world["body"][:2], q_ptr, q_terms, masks=masks, fields=world["values"],
                           mask_id=mask_id, req=None if req is None else pack_pairs(req), exc=None if exc is None else pack_pairs(exc),
                           ranges=ranges, buckets=buckets)


def check(ss_ctx, sc, world, queries, n_masks=3, mask_id=None, req=None, exc=None, clauses=None, buckets=()):
    """host outputs equal the model's counts byte for byte, device outputs equal the host outputs; -> the model's results"""
    import torch
    n_q, n_b = len(queries), len(buckets)
    want = model(world, queries, n_masks, mask_id, req, exc, clauses, buckets)
    q_ptr, q_terms = pack_pairs(queries)
    kw = dict(ranges=None if clauses is None else engine.pack_doc_ranges(clauses), req=None if req is None else pack_pairs(req),
              exc=None if exc is None else pack_pairs(exc), mask_id=mask_id, buckets=list(buckets) if n_b else None)
    # one row more than asked for in every output: it keeps its 0xA5 bytes
    out = (filled(n_q + 1, np.uint32), filled((n_q + 1, max(n_masks, 1)), np.uint32), filled((n_q + 1, max(n_b, 1)), np.uint32))
    sc.facet_counts(q_ptr, q_terms, out=(out[0], out[1] if n_masks else None, out[2] if n_b else None), **kw)
    exp = (filled(n_q + 1, np.uint32), filled((n_q + 1, max(n_masks, 1)), np.uint32), filled((n_q + 1, max(n_b, 1)), np.uint32))
    exp[0][:n_q] = want[0]
    if n_masks:
        exp[1].reshape(-1)[:n_q * n_masks] = want[1].reshape(-1)
    if n_b:
        exp[2].reshape(-1)[:n_q * n_b] = want[2].reshape(-1)
    for name, g, w in zip(("n_match", "mask_counts", "bucket_counts"), out, exp):
        assert g.tobytes() == w.tobytes(), (name, g.reshape(-1)[:16], w.reshape(-1)[:16])
    dev = [torch.full((a.size,), -1515870811, dtype=torch.int32, device="cuda") for a in out]     # 0xA5A5A5A5
    sc.facet_counts(q_ptr, q_terms, out=(dev[0], dev[1] if n_masks else None, dev[2]), **kw)     # (a bucket pointer with n_buckets 0: ignored)
    ss_ctx.synchronize()
    for name, d, h in zip(("n_match", "mask_counts", "bucket_counts"), dev, out):
        assert d.cpu().numpy().tobytes() == h.tobytes(), name
    return want


# ---- the match set ------------------------------------------------------------------------------------------------------------------------

def test_match_set_edges(ss_ctx, world, scorer):
    """title only, body only, both (once), a zero-weight posting, repeats, unknown ids, no usable term, a block no list reaches beside
    one that is hit, postings on the first and last doc of a block and on doc n_docs - 1"""
    queries = [[0], [1], [2], [3], [2, 2, 2], [0, UNKNOWN, 1], [N_TERMS, N_TERMS + 1, UNKNOWN], [], [6], [4], [5], [4, 5], [0, 1, 2, 3, 4, 5],
               [UNKNOWN, 3, N_TERMS, 3]]
    n_match, _, _, sets = check(ss_ctx, scorer, world, queries)
    assert n_match.tolist() == [4, 4, 5, 2, 5, 7, 0, 0, 0, 2, 2, 4, 17, 2]
    assert sets[12][[0, BLOCK - 1, BLOCK, LAST, 900]].all()


def test_more_than_32_lists(ss_ctx, world, scorer):
    """18 terms with a title and a body list each (36 lists), alone and with every other term of the tables: 64 usable terms at most"""
    queries = [BOTH, BOTH + BOTH[::-1], list(range(N_TERMS)), list(range(N_TERMS)) + [UNKNOWN] * 40]
    n_match, _, _, _ = check(ss_ctx, scorer, world, queries, buckets=[(0, 0, 499)])
    assert n_match[0] == n_match[1] and n_match[2] == n_match[3] > n_match[0] > 500


# ---- the allowed set -----------------------------------------------------------------------------------------------------------------------

CONSTRAINT_QUERIES = [[7, 8, 9], [31, 10], [32, 33], [2, 0, 1], [12, 13, 14, 15], [36], [20, 21], [34, 7]]


def constraint_cases():
    n = len(CONSTRAINT_QUERIES)
    none = [[] for _ in range(n)]
    req = [[31], [32], [], [1], [UNKNOWN], [31, 33], [], [35]]
    exc = [[32], [], [31], [UNKNOWN], [12], [], [20], [35]]                     # the last query: a term required AND excluded (no doc)
    one = [[(0, 100, 800)], [], [(1, -1, I64_MAX)], [(0, 0, 999)], [(2, 0, 5000)], [(0, 500, 400)], [(0, 100, 800)], [(0, 100, 800)]]
    four = [[(0, 100, 800), (1, I64_MIN, 1), (2, 100, 100000), (0, 200, 999)]] * 2 + one[2:]
    mask = np.array([0, -1, 1, 2, 2, 0, 0, 1], np.int32)
    shared_req = [[31]] * n                                                     # every query shares ONE allowed set
    return {"mask": dict(mask_id=mask), "req": dict(req=req), "exc": dict(exc=exc), "one-clause": dict(clauses=one),
            "four-clauses": dict(clauses=four), "req+exc": dict(req=req, exc=exc), "all": dict(mask_id=mask, req=req, exc=exc, clauses=four),
            "shared-set": dict(req=shared_req, clauses=[[(0, 100, 800)]] * n), "empty-arrays": dict(req=none, exc=none, clauses=none)}


@pytest.mark.parametrize("case", list(constraint_cases()))
def test_constraints(ss_ctx, world, scorer, case):
    kw = constraint_cases()[case]
    buckets = [(0, 0, 499), (0, 250, 749), (1, I64_MIN, I64_MIN)]
    n_match, mask_counts, bucket_counts, _ = check(ss_ctx, scorer, world, CONSTRAINT_QUERIES, buckets=buckets, **kw)
    free = model(world, CONSTRAINT_QUERIES)[0]
    assert (n_match <= free).all()
    if case != "empty-arrays":
        assert (n_match < free).any() and n_match.sum() > 0                     # the constraint cuts, and not everything
    else:
        assert n_match.tolist() == free.tolist()
    if case in ("all", "req+exc"):
        assert n_match[-1] == 0 and free[-1] > 0                                # required and excluded: CS_EMPTY


# ---- mask counts and buckets ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_masks", [0, 1, 3])
def test_mask_counts(ss_ctx, world, scorer, n_masks):
    scorer.set_doc_masks(world["words"][:n_masks] if n_masks else None)
    queries = [[31], [36, 35], [0, 1], [7], []]
    _, mask_counts, _, _ = check(ss_ctx, scorer, world, queries, n_masks=n_masks, mask_id=None if n_masks == 0 else np.array([0, -1, 0, -1, 0], np.int32))
    if n_masks == 3:                                                            # the mask with garbage past n_docs counts real docs only
        assert mask_counts[2, 2] == np.count_nonzero(world["masks"][2] & world["masks"][0] & model(world, queries)[3][2])


def bucket_cases():
    days = [(0, 990, 999), (0, 900, 999), (0, 500, 999), (0, 0, 999)]           # nested: "past day" .. "past year"
    return {
        "none": [], "one": [(0, 100, 199)], "nested": days, "overlapping": [(0, 0, 600), (0, 400, 999), (0, 500, 500), (0, 400, 999)],
        "two-fields": days[:2] + [(2, 0, 8000), (2, 8001, I64_MAX)] + days[2:], "empty": [(0, 10, 9), (1, I64_MAX, I64_MIN), (0, 0, 999)],
        "extremes": [(1, I64_MIN, I64_MIN), (1, I64_MAX, I64_MAX), (1, I64_MIN, I64_MAX), (1, I64_MIN + 1, I64_MAX - 1), (1, I64_MIN, -1),
                     (1, 0, I64_MAX), (1, I64_MAX - 1, I64_MAX)],
        "max": [(b % 3, 15 * b, 15 * b + 40) if b % 3 != 1 else (1, [I64_MIN, -1, 0, 1][b % 4], [1, I64_MAX][b % 2]) for b in range(MAX_BUCKETS)],
    }


@pytest.mark.parametrize("case", list(bucket_cases()))
def test_buckets(ss_ctx, world, scorer, case):
    buckets = bucket_cases()[case]
    queries = [[31, 32], [36], [7, 8], [0, 1, 2], [], [4]]
    n_match, _, bucket_counts, _ = check(ss_ctx, scorer, world, queries, buckets=buckets, clauses=[[], [(0, 300, 950)], [], [], [], []])
    if case == "nested":
        assert (np.diff(bucket_counts.astype(np.int64), axis=1) >= 0).all() and bucket_counts[0, 3] == n_match[0] and bucket_counts[0, 0] > 0
    if case == "extremes":
        assert bucket_counts[0, 0] > 0 and bucket_counts[0, 1] > 0 and bucket_counts[0, 2] == n_match[0]
    if case == "empty":
        assert bucket_counts[:, :2].sum() == 0
    if case == "max":
        assert len(buckets) == MAX_BUCKETS and np.count_nonzero(bucket_counts[0]) > 40


# ---- agreement with the ranking -------------------------------------------------------------------------------------------------------------

def test_counts_agree_with_ranking(ss_ctx, world, scorer):
    """n_match = n_hits of ss_score_topk_filtered at k = SS_MAX_TOPK with the same arguments; a mask count = n_hits with that mask as the
    query's allow-list; a bucket count = n_hits with the bucket added as a clause.  Every |M(q)| is at most SS_MAX_TOPK."""
    sc = scorer
    queries = [[7, 8, 9], BOTH, [0, 1, 2, 3, 4, 5], [25, 26, 27, 28, 29, 30], [10, 10, UNKNOWN], [], [2], [11, 12, 13, 14], [4], [6, N_TERMS],
               [15, 16], [17, 18, 19, 20]]
    n_q = len(queries)
    req = [[], [], [], [], [], [], [], [11], [], [], [], [17]]
    exc = [[9], [], [5], [], [], [], [], [], [], [], [16], [17]]
    clauses = [[], [(0, 100, 900)], [], [(0, 0, 499), (1, I64_MIN, 1)], [], [], [(0, 0, 999)], [], [], [], [(2, 0, 20000)], []]
    buckets = [(0, 0, 499), (0, 250, 749), (0, 700, 100), (1, I64_MIN, I64_MIN), (1, 0, I64_MAX), (2, 0, 8000)]
    n_match, mask_counts, bucket_counts, _ = check(ss_ctx, sc, world, queries, req=req, exc=exc, clauses=clauses, buckets=buckets)
    assert (n_match <= MAX_TOPK).all() and n_match.max() > 500 and np.count_nonzero(n_match) >= 8      # every query is compared, none skipped
    q_ptr, q_terms = pack_pairs(queries)

    def n_hits(mask_id, cl):
        return sc.score_topk_filtered(q_ptr, q_terms, MAX_TOPK, ranges=engine.pack_doc_ranges(cl), req=pack_pairs(req), exc=pack_pairs(exc),
                                      mask_id=mask_id)[1]

    assert n_hits(None, clauses).tolist() == n_match.tolist()
    for m in range(3):
        assert n_hits(np.full(n_q, m, np.int32), clauses).tolist() == mask_counts[:, m].tolist(), m
    for b, bucket in enumerate(buckets):
        assert n_hits(None, [cl + [bucket] for cl in clauses]).tolist() == bucket_counts[:, b].tolist(), b
    assert mask_counts.sum() > 0 and bucket_counts[:, [0, 1, 4, 5]].sum(axis=0).min() > 0 and bucket_counts[:, 2].sum() == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_outputs_untouched(ss_ctx, world, scorer):
    """invalid ARGUMENTS only: every refusal returns its code and leaves 0xA5 outputs as they were"""
    sc, lib = scorer, ss_ctx.lib
    queries = [[7, 8], [31]]
    q_ptr, q_terms = pack_pairs(queries)
    out = (filled(2, np.uint32), filled((2, 3), np.uint32), filled((2, 2), np.uint32))
    before = [a.tobytes() for a in out]
    two = [(0, 0, 10), (1, 0, 10)]

    def refused(code, q_ptr=q_ptr, q_terms=q_terms, buckets=two, **kw):
        with pytest.raises(SpaghettiError) as ei:
            sc.facet_counts(q_ptr, q_terms, buckets=buckets, out=out, **kw)
        assert ei.value.code == code, (ei.value, kw)
        assert [a.tobytes() for a in out] == before

    refused(ERR_INVALID, q_ptr=np.array([0, 2, 1], np.uint32))                                   # q_ptr decreases
    refused(ERR_INVALID, mask_id=np.array([0, 3], np.int32))                                     # no such mask
    refused(ERR_INVALID, mask_id=np.array([-2, 0], np.int32))
    refused(ERR_INVALID, req=(np.array([1, 1, 1], np.uint32), np.array([7], np.uint32)))         # req_ptr does not start at 0
    refused(ERR_INVALID, exc=(np.array([0, 1, 0], np.uint32), np.array([7], np.uint32)))         # exc_ptr decreases
    refused(ERR_UNSUPPORTED, req=pack_pairs([list(range(17)), []]))                              # 17 distinct constraint terms
    refused(ERR_INVALID, ranges=engine.pack_doc_ranges([[(3, 0, 1)], []]))                       # a clause on a field that is not there
    refused(ERR_INVALID, ranges=(np.array([0, 1, 0], np.uint32), engine.pack_doc_ranges([[(0, 0, 1)]])[1]))
    refused(ERR_UNSUPPORTED, ranges=engine.pack_doc_ranges([[(0, 0, 1)] * 5, []]))               # five clauses
    refused(ERR_INVALID, buckets=[(0, 0, 1), (3, 0, 1)])                                         # a bucket on a field that is not there
    refused(ERR_INVALID, buckets=[(-1, 0, 1)])
    # the raw ABI: NULL pointers and negative counts
    ptr = lambda a: a.ctypes.data                                                                 # noqa: E731
    bk = engine.pack_doc_ranges([two])[1]
    args = lambda **o: [o.get("s", sc.h), o.get("n_q", 2), o.get("q_ptr", ptr(q_ptr)), o.get("q_terms", ptr(q_terms)), None, None, None, None, None,   # noqa: E731
                        None, None, o.get("n_b", 2), o.get("bk", ptr(bk)), o.get("n_match", ptr(out[0])), ptr(out[1]), o.get("b_out", ptr(out[2]))]
    for code, o in ((ERR_INVALID, dict(s=None)), (ERR_INVALID, dict(n_q=-1)), (ERR_INVALID, dict(q_ptr=None)), (ERR_INVALID, dict(q_terms=None)),
                    (ERR_INVALID, dict(n_match=None)), (ERR_INVALID, dict(n_b=-1)), (ERR_INVALID, dict(bk=None)), (ERR_INVALID, dict(b_out=None)),
                    (ERR_UNSUPPORTED, dict(n_b=MAX_BUCKETS + 1))):
        assert lib.ss_facet_counts(*args(**o)) == code, o
        assert [a.tobytes() for a in out] == before
    assert lib.ss_facet_counts(*args(n_q=0)) == 0 and [a.tobytes() for a in out] == before       # n_q == 0: SS_OK, nothing done
    # more than SS_MAX_QUERY_TERMS distinct usable terms need a larger vocabulary than this world's: test_too_many_query_terms
    sc.set_doc_fields(None)                                                                      # a bucket, a clause, but no field table
    refused(ERR_STATE)
    refused(ERR_STATE, buckets=None, ranges=engine.pack_doc_ranges([[(0, 0, 1)], []]))
    got = sc.facet_counts(q_ptr, q_terms, buckets=None, out=(out[0], out[1], None))              # ... and without either the call stands
    assert got[0].tolist() == model(world, queries)[0].tolist()


def test_too_many_query_terms(ss_ctx):
    """65 distinct usable terms in one query are refused as the scoring calls refuse them; 64 are counted"""
    n_docs, n_terms = 40, 70
    ptr = np.arange(n_terms + 1, dtype=np.uint64)
    doc = (np.arange(n_terms) % n_docs).astype(np.uint32)
    table = (ptr, doc, np.ones(n_terms, np.float32))
    sc, ti, bi = make_scorer(ss_ctx, n_docs, table, table, np.ones(n_docs), np.ones(n_docs))
    try:
        out = (filled(1, np.uint32), None, None)
        with pytest.raises(SpaghettiError) as ei:
            sc.facet_counts(np.array([0, 65], np.uint32), np.arange(65, dtype=np.uint32), out=out)
        assert ei.value.code == ERR_UNSUPPORTED and out[0].tobytes() == bytes([FILL]) * 4
        n_match = sc.facet_counts(np.array([0, 66], np.uint32), np.concatenate([np.arange(64), [0, UNKNOWN]]).astype(np.uint32))[0]
        assert n_match.tolist() == [40]
    finally:
        close_all(sc, ti, bi)
