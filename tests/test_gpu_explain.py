"""GPU parity: "explain hits" (ss_explain_hits) vs the numpy model (tests/explain_model.explain_ref).  Every comparison is bit-exact:
tobytes() on whole output arrays that start from 0xA5 bytes, so an entry the call must not write is checked with the ones it must.
"""
import os

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import explain_model as xm
from tests.test_explain_cpu import HAND_BODY, HAND_POS, HAND_TITLE, positions_of
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)
from tests.test_gpu_score import close_all, make_scorer
from tests.test_related_terms_cpu import table_of

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 7
UNKNOWN = 0xFFFFFFFF
FILL = 0xA5
F32 = np.float32
NAN = float("nan")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_300x80.npz")


def prefilled(n_q, k, t_stride):
    return np.frombuffer(bytes([FILL]) * (n_q * k * t_stride * 16), dtype=engine.TERM_MATCH_DTYPE).reshape(n_q, k, t_stride).copy()


def explain(sc, q_ptr, q_terms, hits, n_hits, t_stride):
    n_q, k = hits.shape
    return sc.explain_hits(q_ptr, q_terms, hits, n_hits, t_stride=t_stride, out=prefilled(n_q, k, t_stride))


def made_up(docs_rows, k=None):
    """lists of doc ids -> (hits [n_q][k] with nothing but .doc set, n_hits); slots behind a row's last hit name doc 0"""
    k = k or max(1, max(len(r) for r in docs_rows))
    hits = np.zeros((len(docs_rows), k), dtype=engine.HIT_DTYPE)
    for q, r in enumerate(docs_rows):
        hits["doc"][q, :len(r)] = r
    return hits, np.array([len(r) for r in docs_rows], np.int32)


def queries(rows):
    q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return q_ptr, np.array([t for r in rows for t in r], dtype=np.uint32)


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


@pytest.fixture(scope="module")
def world():
    """The golden 300 x 80 tables with their stored weights, positions for both tables (every 9th body list long), and a batch that
    mixes 1-, 3- and 12-token queries: head terms, a duplicated token, unknown ids, and one query of unknown terms only (no hits)."""
    z = np.load(GOLDEN)
    n_docs, n_terms = int(z["n_docs"]), len(z["b_ptr"]) - 1
    title, body = (z["t_ptr"], z["t_doc"], z["t_w"]), (z["b_ptr"], z["b_doc"], z["b_w"])
    rows = [[3], [0, 1, 2], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [UNKNOWN, n_terms], [70, 5, 70],
            [79, 40, UNKNOWN, 1, 1, n_terms, 33, 2, 60, 0, 79, 12], [50]]
    q_ptr, q_terms = queries(rows)
    return {"n_docs": n_docs, "n_terms": n_terms, "title": title, "body": body, "mt": z["t_mag"], "mb": z["b_mag"],
            "tpos": random_positions(len(z["t_doc"]), 7), "bpos": random_positions(len(z["b_doc"]), 8, long_every=9),
            "q_ptr": q_ptr, "q_terms": q_terms, "longest": 12}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, world["n_docs"], world["title"], world["body"], world["mt"], world["mb"])
    ti.set_positions(*world["tpos"])
    bi.set_positions(*world["bpos"])
    yield sc, ti, bi
    close_all(sc, ti, bi)


def model(world, q_ptr, q_terms, hits, n_hits, t_stride, body_pos="world"):
    return xm.explain_ref(world["title"], world["body"], world["n_docs"], q_ptr, q_terms, hits["doc"], n_hits, t_stride,
                          body_pos=world["bpos"] if isinstance(body_pos, str) else body_pos, fill=FILL)


# k = 40: the 12-token query has more than 256 entries, the kernel's workgroup; t_stride: the longest query exactly, and larger
@pytest.mark.parametrize("k,t_stride", [(1, 12), (10, 12), (10, 17), (40, 12)])
def test_rows_of_score_topk_equal_the_model(ss_ctx, world, scorer, k, t_stride):
    import torch
    sc, ti, bi = scorer
    q_ptr, q_terms = world["q_ptr"], world["q_terms"]
    n_q = len(q_ptr) - 1
    hits, n_hits = sc.score_topk(q_ptr, q_terms, k)
    assert n_hits[3] == 0 and n_hits[2] == k and (k < 40 or int(n_hits[2]) * 12 > 256)
    want = model(world, q_ptr, q_terms, hits, n_hits, t_stride)
    assert want[3].tobytes() == bytes([FILL]) * (k * t_stride * 16)          # the query without hits: nothing is written
    # host hits and out
    got = explain(sc, q_ptr, q_terms, hits, n_hits, t_stride)
    assert got.tobytes() == want.tobytes()
    # the default t_stride is the longest query; a fresh array starts from zeros
    if t_stride == world["longest"]:
        dflt = sc.explain_hits(q_ptr, q_terms, hits, n_hits)
        assert dflt.shape == (n_q, k, 12)
        assert dflt.tobytes() == xm.explain_ref(world["title"], world["body"], world["n_docs"], q_ptr, q_terms, hits["doc"], n_hits, 12,
                                                body_pos=world["bpos"]).tobytes()
    # everything in device memory: the call sits between the scoring call and ss_synchronize, nothing waits in between.  Four
    # rounds — more than the scorer has turns — so that the pinned blocks of the queries' table come round again while in flight;
    # odd rounds explain a batch of other queries (the first three, reversed tokens) into a buffer of their own.
    lib = ss_ctx.lib
    qp2, qt2 = queries([[3], [2, 1, 0], list(range(11, -1, -1))])
    d_hits = [torch.zeros(n_q * k * 40, dtype=torch.uint8, device="cuda") for _ in range(4)]
    d_n = [torch.zeros(n_q, dtype=torch.int32, device="cuda") for _ in range(4)]
    d_out = [torch.full((n_q * k * t_stride * 16,), FILL, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for r in range(4):
        qp, qt, nq = (q_ptr, q_terms, n_q) if r % 2 == 0 else (qp2, qt2, 3)
        rc = lib.ss_score_topk(sc.h, nq, qp.ctypes.data, qt.ctypes.data, None, None, k, d_hits[r].data_ptr(), d_n[r].data_ptr())
        assert rc == 0
        rc = lib.ss_explain_hits(sc.h, nq, qp.ctypes.data, qt.ctypes.data, k, d_hits[r].data_ptr(), d_n[r].data_ptr(), t_stride,
                                 d_out[r].data_ptr())
        assert rc == 0
    ss_ctx.synchronize()
    for r in range(4):
        rows = d_hits[r].cpu().numpy().view(engine.HIT_DTYPE).reshape(n_q, k)
        if r % 2 == 0:
            assert rows.tobytes() == hits.tobytes() and d_n[r].cpu().numpy().tolist() == n_hits.tolist()
            assert d_out[r].cpu().numpy().tobytes() == want.tobytes(), r
        else:
            want2 = model(world, qp2, qt2, rows[:3], d_n[r].cpu().numpy()[:3], t_stride)
            assert d_out[r].cpu().numpy()[:3 * k * t_stride * 16].tobytes() == want2.tobytes(), r
            assert (d_out[r].cpu().numpy()[3 * k * t_stride * 16:] == FILL).all()
    # a device n_hits outside [0, k] is clamped by the kernel (host: refused, see the refusals test); mixed host / device arrays work
    d_bad = torch.tensor([k + 5, -3] + [0] * (n_q - 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = sc.explain_hits(q_ptr, q_terms, hits, d_bad, t_stride=t_stride, out=prefilled(n_q, k, t_stride))
    clamped = np.array([k, 0] + [0] * (n_q - 2), np.int32)
    assert got.tobytes() == model(world, q_ptr, q_terms, hits, clamped, t_stride).tobytes()


def test_turn_blocks_regrown_under_queued_calls(ss_ctx, world, scorer):
    """Seven device-only calls back to back, more than twice the scorer's three turns, nothing waited for in between.  The batches
    hold 3, 40, 7, 64, 1, 64 and 5 queries (windows of the world's seven queries taken round and round), so the calls of 64 meet their
    turn's pinned block and device copy too small and replace them while the two calls before them are still queued.  Every output
    then equals the host-output call on the same window, byte for byte."""
    import torch
    sc, ti, bi = scorer
    lib = ss_ctx.lib
    k, t_stride = 10, world["longest"]
    seven = [world["q_terms"][world["q_ptr"][q]:world["q_ptr"][q + 1]].tolist() for q in range(7)]
    q_ptr, q_terms = queries([seven[i % 7] for i in range(64)])
    hits, n_hits = sc.score_topk(q_ptr, q_terms, k)
    calls = []
    for n, first in zip((3, 40, 7, 64, 1, 64, 5), (0, 11, 50, 0, 33, 0, 20)):
        qp = (q_ptr[first:first + n + 1] - q_ptr[first]).astype(np.uint32)
        qt = np.ascontiguousarray(q_terms[q_ptr[first]:q_ptr[first + n]])
        h, nh = np.ascontiguousarray(hits[first:first + n]), np.ascontiguousarray(n_hits[first:first + n])
        calls.append({"n": n, "qp": qp, "qt": qt, "h": h, "nh": nh,
                      "d_h": torch.from_numpy(h.view(np.uint8).reshape(-1)).cuda(), "d_nh": torch.from_numpy(nh).cuda(),
                      "d_out": torch.full((n * k * t_stride * 16,), FILL, dtype=torch.uint8, device="cuda")})
    torch.cuda.synchronize()
    for c in calls:
        rc = lib.ss_explain_hits(sc.h, c["n"], c["qp"].ctypes.data, c["qt"].ctypes.data, k, c["d_h"].data_ptr(), c["d_nh"].data_ptr(),
                                 t_stride, c["d_out"].data_ptr())
        assert rc == 0
    ss_ctx.synchronize()
    assert any(int(c["nh"].sum()) > 0 for c in calls)
    for i, c in enumerate(calls):
        want = explain(sc, c["qp"], c["qt"], c["h"], c["nh"], t_stride)
        assert c["d_out"].cpu().numpy().tobytes() == want.tobytes(), i


def edge_tables():
    """700 docs, 4 terms.  body: term 0 no postings, term 1 one posting (doc 5), term 2 every even doc from 10 to 608 (300 postings:
    more than three times the wave width, the widest granule of the kernel), term 3 every doc.  title: term 2 every third doc."""
    n_docs = 700
    b_lists = [[], [5], list(range(10, 610, 2)), list(range(n_docs))]
    t_lists = [[0], [], list(range(0, n_docs, 3)), [n_docs - 1]]

    def table(lists, seed):
        rng = np.random.default_rng(seed)
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
        doc = np.array([d for x in lists for d in x], dtype=np.uint32)
        return ptr, doc, (1.0 + rng.random(len(doc))).astype(np.float32)
    return n_docs, table(t_lists, 1), table(b_lists, 2)


def test_list_edges_and_defined_non_errors(ss_ctx):
    """Every doc id of the corpus, n_docs and 0xFFFFFFFF as made-up hits against lists of length 0, 1, 300 and n_docs: the first and
    the last posting of a list, ids between two postings and beyond the last one, every position of the long list (so every 64-posting
    seam and its neighbours), with an unknown term and the id n_terms among the tokens."""
    n_docs, title, body = edge_tables()
    bpos = random_positions(len(body[1]), 3, long_every=50)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, np.ones(n_docs), np.ones(n_docs))
    try:
        bi.set_positions(*bpos)
        probes = list(range(n_docs)) + [n_docs, UNKNOWN]
        hits, n_hits = made_up([probes, [608, 609, 610, 9, 10, 11, 5, 4, 6, 0, n_docs - 1]], k=len(probes))
        q_ptr, q_terms = queries([[2, UNKNOWN, 0, 4, 1, 3], [2, 1, 3]])
        got = explain(sc, q_ptr, q_terms, hits, n_hits, 6)
        want = xm.explain_ref(title, body, n_docs, q_ptr, q_terms, hits["doc"], n_hits, 6, body_pos=bpos, fill=FILL)
        assert got.tobytes() == want.tobytes()
        f = got["flags"]
        # the long list: first posting (doc 10), last (608), between two (11), beyond the last (609, 610), before the first (9)
        assert (f[1, [0, 4], 0] & 2).all() and not (f[1, [1, 2, 3, 5], 0] & 2).any()
        assert [int(x & 2) for x in f[0, 8:612, 0]] == [2 if 10 <= d <= 608 and d % 2 == 0 else 0 for d in range(8, 612)]
        # lists of length 0 and 1
        assert not (f[0, :n_docs, 2] & 2).any() and [d for d in range(n_docs) if f[0, d, 4] & 2] == [5]
        # the unknown term, the id n_terms, the doc n_docs and the doc 0xFFFFFFFF: all zero, between neighbours that are not
        zero = bytes(16)
        assert all(got[0, d, i].tobytes() == zero for d in range(n_docs + 2) for i in (1, 3))
        assert all(got[0, d, i].tobytes() == zero for d in (n_docs, n_docs + 1) for i in range(6))
        assert f[0, n_docs - 1, 5] & 3 == 3 and f[0, n_docs - 2, 5] & 3 == 2          # term 3: every doc's body, the last doc's title
    finally:
        close_all(sc, ti, bi)


def test_stored_bits(ss_ctx):
    """-0.0, +0.0 and NaN weights come back bit for bit with their flag set"""
    w = [F32(-0.0), F32(0.0), F32(NAN), F32(2.5)]
    title = table_of([{0: w[d % 4]} for d in range(8)], 2)
    body = table_of([{0: w[(d + 1) % 4], 1: w[(d + 2) % 4]} if d < 6 else {} for d in range(8)], 2)
    sc, ti, bi = make_scorer(ss_ctx, 8, title, body, np.ones(8), np.ones(8))
    try:
        hits, n_hits = made_up([list(range(8))])
        q_ptr, q_terms = queries([[0, 1]])
        got = explain(sc, q_ptr, q_terms, hits, n_hits, 2)
        assert got.tobytes() == xm.explain_ref(title, body, 8, q_ptr, q_terms, hits["doc"], n_hits, 2, fill=FILL).tobytes()
        assert got["flags"][0, :, 0].tolist() == [3] * 6 + [1] * 2 and got["flags"][0, :, 1].tolist() == [2] * 6 + [0] * 2
        assert got["title_w"][0, :, 0].tobytes() == np.array([w[d % 4] for d in range(8)], np.float32).tobytes()
        assert got["body_w"][0, :6, 0].tobytes() == np.array([w[(d + 1) % 4] for d in range(6)], np.float32).tobytes()
        assert got["body_w"][0, :6, 1].tobytes() == np.array([w[(d + 2) % 4] for d in range(6)], np.float32).tobytes()
        assert got["body_w"][0, 6:].tobytes() == bytes(16) and got["title_w"][0, :, 1].tobytes() == bytes(32)
    finally:
        close_all(sc, ti, bi)


def test_positions(ss_ctx):
    """The hand-worked lists of test_explain_cpu.py, then lists around the length one lane reads alone (16) and around the wave width,
    each with its minimum LAST, several of them in one wave; then a body table without positions, with and without title positions."""
    title, body = table_of(HAND_TITLE, 4), table_of(HAND_BODY, 4)
    pos = positions_of(HAND_POS)
    sc, ti, bi = make_scorer(ss_ctx, 5, title, body, np.ones(5), np.ones(5))
    try:
        hits, n_hits = made_up([[0, 1, 2, 3, 4]])
        q_ptr, q_terms = queries([[0, 2]])
        no_pos = explain(sc, q_ptr, q_terms, hits, n_hits, 2)
        assert not (no_pos["flags"] & 4).any() and not no_pos["body_pos"].view(np.uint32).any()
        assert no_pos.tobytes() == xm.explain_ref(title, body, 5, q_ptr, q_terms, hits["doc"], n_hits, 2, fill=FILL).tobytes()
        ti.set_positions(*positions_of([[1.0], [2.0], [3.0]]))              # title positions alone change nothing
        assert explain(sc, q_ptr, q_terms, hits, n_hits, 2).tobytes() == no_pos.tobytes()
        bi.set_positions(*pos)
        got = explain(sc, q_ptr, q_terms, hits, n_hits, 2)
        assert got.tobytes() == xm.explain_ref(title, body, 5, q_ptr, q_terms, hits["doc"], n_hits, 2, body_pos=pos, fill=FILL).tobytes()
        # term 0: doc 1 [7, 2], doc 2 [];  term 2: doc 0 [-100], doc 1 [NaN, 7, 3], doc 2 [-100, 0], doc 3 [4]
        assert (got["flags"][0] & 4).tolist() == [[0, 0], [4, 4], [0, 4], [0, 4], [0, 0]]
        assert got["body_pos"][0].tolist() == [[0.0, 0.0], [2.0, 3.0], [0.0, 0.0], [0.0, 4.0], [0.0, 0.0]]
    finally:
        close_all(sc, ti, bi)
    # one term in 40 docs; doc d's list has LENGTHS[d % 10] values: 1000 + 3 * x descending after a NaN and a -100, so the smallest
    # value >= 0 sits last; doc 39's values are negative or NaN only
    lengths = [15, 16, 17, 63, 64, 65, 200, 129, 3, 1000]
    lists = []
    for d in range(40):
        n = lengths[d % 10]
        vals = [NAN, -100.0] + [1000.0 + 3 * (n - x) + d for x in range(n - 2)] if n > 2 else [5.0] * n
        lists.append(vals[:n] if d < 39 else [NAN if x % 2 else -1.0 for x in range(n)])
    body = table_of([{0: 1.0} for _ in range(40)], 1)
    title = table_of([{} for _ in range(40)], 1)
    pos = positions_of(lists)
    sc, ti, bi = make_scorer(ss_ctx, 40, title, body, np.ones(40), np.ones(40))
    try:
        bi.set_positions(*pos)
        hits, n_hits = made_up([list(range(40))])
        q_ptr, q_terms = queries([[0]])
        got = explain(sc, q_ptr, q_terms, hits, n_hits, 1)
        assert got.tobytes() == xm.explain_ref(title, body, 40, q_ptr, q_terms, hits["doc"], n_hits, 1, body_pos=pos, fill=FILL).tobytes()
        assert got["flags"][0, :, 0].tolist() == [6] * 39 + [2]
        assert got["body_pos"][0, :39, 0].tolist() == [float(F32(lists[d][-1])) for d in range(39)]
    finally:
        close_all(sc, ti, bi)


def test_rows_of_the_other_scoring_calls(ss_ctx, world, scorer):
    """masked, constrained, phrase and similar-pages rows explained: the model on their docs; a constrained row's hits hold every
    required term and no excluded one"""
    sc, ti, bi = scorer
    n_docs, k = world["n_docs"], 10
    q_ptr, q_terms = queries([[0, 1, 2], [5, 9, 20, 3], [7]])
    # masked
    rng = np.random.default_rng(5)
    sc.set_doc_masks(engine.pack_doc_masks(rng.random((1, n_docs)) < 0.5, n_docs))
    hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, np.array([0, -1, 0], np.int32), k)
    assert explain(sc, q_ptr, q_terms, hits, n_hits, 4).tobytes() == model(world, q_ptr, q_terms, hits, n_hits, 4).tobytes()
    # constrained: +1 -2 on query 0, +9 on query 1, -7's neighbour 8 on query 2; the constraint terms ride along as tokens
    req, exc = queries([[1], [9], []]), queries([[2], [], [8]])
    hits, n_hits = sc.score_topk_constrained(q_ptr, q_terms, k, req=req, exc=exc)
    assert (n_hits > 0).all()
    xq_ptr, xq_terms = queries([[0, 1, 2], [5, 9, 20, 3], [7, 8]])
    got = explain(sc, xq_ptr, xq_terms, hits, n_hits, 4)
    assert got.tobytes() == model(world, xq_ptr, xq_terms, hits, n_hits, 4).tobytes()
    f = got["flags"] & 3
    assert f[0, :n_hits[0], 1].all() and not f[0, :n_hits[0], 2].any() and f[1, :n_hits[1], 1].all() and not f[2, :n_hits[2], 1].any()
    # phrase: the phrase's words as further tokens
    p_ptr, p_terms = queries([[0, 1], [], [2, 3]])
    hits, n_hits = sc.score_topk_phrase(q_ptr, q_terms, p_ptr, p_terms, k)
    pq_ptr, pq_terms = queries([[0, 1, 2, 0, 1], [5, 9, 20, 3], [7, 2, 3]])
    assert explain(sc, pq_ptr, pq_terms, hits, n_hits, 5).tobytes() == model(world, pq_ptr, pq_terms, hits, n_hits, 5).tobytes()
    # similar pages: the seed's heaviest body terms are the query
    bi.build_doc_view()
    seeds = np.array([3, 150, 299], np.uint32)
    hits, n_hits = sc.similar_topk(seeds, k, m=5)
    terms, _, cnt = bi.doc_top_terms(seeds, 5)
    sq_ptr, sq_terms = queries([terms[q, :cnt[q]].tolist() for q in range(3)])
    got = explain(sc, sq_ptr, sq_terms, hits, n_hits, 5)
    assert got.tobytes() == model(world, sq_ptr, sq_terms, hits, n_hits, 5).tobytes()
    assert (n_hits > 0).all() and all((got["flags"][q, j, :cnt[q]] & 3).any() for q in range(3) for j in range(n_hits[q]))


def test_final_rank_recomputed_from_the_entries(ss_ctx):
    """Phrase-free queries on a clean table: FinalRank recomputed in float64 from the explain entries and ss_index_read_magnitudes, in
    the expression order of final_rank (score_common.hpp), equals hit.final bit for bit.  The weights are multiples of 2^-10 below 8:
    a sum of up to 64 of them is a multiple of 2^-10 below 2^9, i.e. 19 significant bits — exact in float64 in any order."""
    rng = np.random.default_rng(11)
    n_docs, n_terms = 300, 80

    def table(p):
        rows = [{int(t): float(rng.integers(256, 8192)) / 1024.0 for t in np.nonzero(rng.random(n_terms) < p)[0]} for _ in range(n_docs)]
        return table_of(rows, n_terms)
    title, body = table(0.03), table(0.15)
    for w in (title[2], body[2]):
        scaled = w.astype(np.float64) * 1024.0
        assert (scaled == np.round(scaled)).all() and (scaled < 8192).all() and (scaled >= 256).all()
    mt, mb = 0.5 + rng.random(n_docs) * 8.0, 0.5 + rng.random(n_docs) * 8.0
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        rows = [[4], [0, 1, 2], [3, 9, 9, 17, 2, 40, 41, 42, 43, 5, 6, 3], [70, UNKNOWN, 71]]
        q_ptr, q_terms = queries(rows)
        hits, n_hits = sc.score_topk(q_ptr, q_terms, 10)
        got = explain(sc, q_ptr, q_terms, hits, n_hits, 12)
        checked = 0
        for q, toks in enumerate(rows):
            qmag = np.sqrt(np.float64(len(toks)))
            assert n_hits[q] > 0
            docs = np.ascontiguousarray(hits["doc"][q, :n_hits[q]])
            m_t, m_b = ti.read_magnitudes(docs), bi.read_magnitudes(docs)
            assert m_t.tobytes() == mt[docs].tobytes() and m_b.tobytes() == mb[docs].tobytes()
            for j in range(int(n_hits[q])):
                T = sum(np.float64(x) for x in got["title_w"][q, j, :len(toks)])
                B = sum(np.float64(x) for x in got["body_w"][q, j, :len(toks)])
                bodyr, titler = np.float64(B) / (m_b[j] * qmag), np.float64(T) / (m_t[j] * qmag)
                fin = (0.33 * 0.0 + 0.38 * titler + 0.29 * bodyr) * 100.0
                assert np.float64(fin).tobytes() == hits["final"][q, j].tobytes(), (q, j)
                assert np.float64(titler).tobytes() == hits["title"][q, j].tobytes() and np.float64(bodyr).tobytes() == hits["body"][q, j].tobytes()
                checked += 1
        assert checked >= 25
    finally:
        close_all(sc, ti, bi)


def test_refusals_leave_out_untouched(ss_ctx, world, scorer):
    sc, ti, bi = scorer
    lib = ss_ctx.lib
    q_ptr, q_terms = queries([[0, 1, 2], [3]])
    hits, n_hits = sc.score_topk(q_ptr, q_terms, 4)
    out = prefilled(2, 4, 3)

    def call(code, handle=None, n_q=2, qp=q_ptr, qt=q_terms, k=4, h=hits, n=n_hits, t_stride=3, o=out):
        ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
        rc = lib.ss_explain_hits(sc.h if handle is None else handle, n_q, ptr(qp), ptr(qt), k, ptr(h), ptr(n), t_stride, ptr(o))
        assert rc == code, (rc, code)
        assert (out.view(np.uint8) == FILL).all()
    assert lib.ss_explain_hits(None, 2, q_ptr.ctypes.data, q_terms.ctypes.data, 4, hits.ctypes.data, n_hits.ctypes.data, 3, out.ctypes.data) == ERR_INVALID
    assert (out.view(np.uint8) == FILL).all()
    call(ERR_INVALID, o=None)
    call(ERR_INVALID, n_q=-1)
    call(ERR_INVALID, k=0)
    call(ERR_INVALID, t_stride=0)
    call(ERR_INVALID, qp=None)
    call(ERR_INVALID, qp=np.array([0, 3, 2], np.uint32))
    call(ERR_INVALID, qt=None)
    call(ERR_INVALID, h=None)
    call(ERR_INVALID, n=None)
    call(ERR_INVALID, t_stride=2)                                       # query 0 has three tokens
    call(ERR_UNSUPPORTED, k=1025)
    call(ERR_UNSUPPORTED, t_stride=65)
    call(ERR_UNSUPPORTED, n_q=32768, k=1024, t_stride=64, qp=np.zeros(32769, np.uint32))      # 2^31 entries
    call(ERR_INVALID, n=np.array([5, 1], np.int32))
    call(ERR_INVALID, n=np.array([1, -1], np.int32))
    call(0, n_q=0)                                                      # nothing to do: SS_OK, nothing written
    with pytest.raises(SpaghettiError) as ei:
        sc.explain_hits(q_ptr, q_terms, hits, n_hits, t_stride=2, out=out)
    assert ei.value.code == ERR_INVALID and (out.view(np.uint8) == FILL).all()
    # and the same arguments untouched are accepted
    call_ok = explain(sc, q_ptr, q_terms, hits, n_hits, 3)
    assert call_ok.tobytes() == model(world, q_ptr, q_terms, hits, n_hits, 3).tobytes()


def test_host_mirror_explain_results(host, corpus):
    """DeviceIndex.ExplainResults on the config-1 corpus of test_gpu_host.py: matched and missing words and the earliest position of
    every row RetrieveBatch returned, against the corpus' own posting maps."""
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    di = host.DeviceIndex()
    di.load(forw, inv)

    def check(query, words, rows):
        ex = di.ExplainResults(query, rows)
        assert len(ex) == len(rows)
        seen = {"title": 0, "body": 0, "missing": 0, "pos": 0}
        for r, e in zip(rows, ex):
            uniq = list(dict.fromkeys(words))
            in_t = [h(w) for w in uniq if r.DocHash in corpus["title"].get(h(w), {})]
            in_b = [h(w) for w in uniq if r.DocHash in corpus["body"].get(h(w), {})]
            assert e.TitleWords == in_t and e.BodyWords == in_b
            assert e.MissingWords == [h(w) for w in uniq if h(w) not in in_t and h(w) not in in_b]
            firsts = [xm.earliest_position(corpus["body"][h(w)][r.DocHash][1:]) for w in uniq if h(w) in in_b]
            firsts = [float(x) for x in firsts if x is not None]
            assert e.FirstPosition == (min(firsts) if firsts else None)
            seen["title"] += bool(in_t)
            seen["body"] += bool(in_b)
            seen["missing"] += bool(e.MissingWords)
            seen["pos"] += e.FirstPosition is not None
        return seen
    query = "w3 w40 w149 notaword w3"
    rows = di.RetrieveBatch([query], 30)[0]
    seen = check(query, ["w3", "w40", "w149", "notaword", "w3"], rows)
    assert len(rows) == 30 and seen["body"] > 0 and seen["missing"] == 30 and seen["pos"] > 0
    # title hits (anchor words of uncrawled children: no body posting, no position), and a phrase whose words count as tokens
    seen = check("w120", ["w120"], di.RetrieveBatch(["w120"], 50)[0])
    assert seen["title"] > 0
    query = 'w7 "w1 w2"'
    check(query, ["w7", "w1", "w2"], di.RetrieveBatch([query], 20)[0])
    # operators are read only when switched on: '-w40' is then no token, '+w3' a plain word
    query = "+w3 -w40"
    rows = di.RetrieveBatch([query], 20)[0]
    check(query, ["w3", "w40"], rows)
    di.SetQueryOperators(True)
    rows = di.RetrieveBatch([query], 20)[0]
    seen = check(query, ["w3"], rows)
    assert len(rows) > 0 and seen["missing"] == 0
    di.SetQueryOperators(False)
    # a row the index does not know lacks every word; no rows, no words
    rows = di.RetrieveBatch(["w3"], 2)[0]
    assert di.ExplainResults("w3", []) == [] and [e.MissingWords for e in di.ExplainResults("", rows)] == [[], []]
