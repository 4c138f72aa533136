"""GPU parity: "related terms" (ss_related_terms) vs the numpy model over the CPU oracle's rows (tests/related_terms_model.related_ref)
and vs the same model fed from the public calls (ss_score_topk[_masked] -> ss_index_doc_top_terms).  Every comparison is
bit-exact: tobytes() on the terms, the counts and the scores' bits.
"""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import doc_view_model as dvm
from tests import related_terms_model as rtm
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)
from tests.test_gpu_score import assert_same_hits, build_weighted, close_all, make_scorer
from tests.test_related_terms_cpu import HAND_DOCS, table_of

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 6
N_DOCS, N_TERMS, K_TOPICS = 20000, 1000, 8
UNKNOWN = 0xFFFFFFFF


@pytest.fixture(autouse=True, params=[0, 1], ids=["small-kernel-off", "small-kernel-on"])
def _small_query_routing(request, ss_ctx):
    """As in test_gpu_similar.py: every test runs with k_score_small off and with every query that fits sent there."""
    ss_ctx.set_option("score.small", request.param)
    yield
    ss_ctx.set_option("score.small", None)


def same(got, want):
    """(terms, score, n_out) twice: identical bytes, entries past n_out included (both sides start from zeros)"""
    assert got[2].tolist() == want[2].tolist()
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


def make_queries(title, body):
    """64 queries of 1 - 4 terms: head terms, tail terms, one of unknown terms only, one with a duplicated term, one whose only term
    is the rarest of the tables (fewer matching docs than the largest k_fb)."""
    rng = np.random.default_rng(41)
    df = np.diff(np.asarray(body[0]).astype(np.int64)) + np.diff(np.asarray(title[0]).astype(np.int64))
    rare = int(np.argmin(df))
    assert 0 < df[rare] < engine._lib.SS_MAX_FEEDBACK_DOCS
    qs = []
    for q in range(61):
        n = int(rng.integers(1, 5))
        pool = (0, 20) if q % 3 == 0 else (N_TERMS - 200, N_TERMS) if q % 3 == 1 else (0, N_TERMS)      # head, tail, anything
        qs.append(rng.choice(np.arange(*pool), size=n, replace=False).tolist())
    qs.append([UNKNOWN, UNKNOWN - 1])
    qs.append([7, 300, 7])
    qs.append([rare])
    q_ptr = np.concatenate([[0], np.cumsum([len(x) for x in qs])]).astype(np.uint32)
    return q_ptr, np.array([t for x in qs for t in x], dtype=np.uint32)


@pytest.fixture(scope="module")
def world(oracle):
    """The tables of test_gpu_similar.py, the queries, the prior and the body view of the model, built once."""
    title, body, mt, mb = build_weighted(oracle, N_DOCS, N_TERMS, 200000, 20000, 3)
    q_ptr, q_terms = make_queries(title, body)
    rng = np.random.default_rng(42)
    prior = rng.random((K_TOPICS, N_DOCS)) * 50.0
    probs = rng.dirichlet(np.ones(K_TOPICS), size=len(q_ptr) - 1)
    return {"title": title, "body": body, "mt": mt, "mb": mb, "q_ptr": q_ptr, "q_terms": q_terms, "prior": prior, "probs": probs,
            "view": dvm.doc_view(*body, N_DOCS), "refs": {}}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, N_DOCS, world["title"], world["body"], world["mt"], world["mb"])
    bi.build_doc_view()
    yield sc, ti, bi
    close_all(sc, ti, bi)


def reference(oracle, world, k_fb, m_doc, m, with_prior):
    """related_ref over the oracle's rows, computed once per case and shared by the two routings"""
    key = (k_fb, m_doc, m, with_prior)
    if key not in world["refs"]:
        kw = {"prior": np.ascontiguousarray(world["prior"].T), "topic_probs": world["probs"]} if with_prior else {}
        rows, n_rows = oracle.score_topk_batch(N_DOCS, world["title"], world["body"], world["mt"], world["mb"], world["q_ptr"],
                                               world["q_terms"], k_fb, **kw)
        world["refs"][key] = (rtm.related_ref(rows, n_rows, world["view"], world["q_ptr"], world["q_terms"], m_doc, m), n_rows)
    return world["refs"][key]


def composed(sc, bi, q_ptr, q_terms, k_fb, m_doc, m, topic_probs=None, mask_id=None):
    """the definition through the public calls: the scoring call at k_fb, then ss_index_doc_top_terms of every hit, then the model's
    sums and order"""
    if mask_id is None:
        rows, n_rows = sc.score_topk(q_ptr, q_terms, k_fb, topic_probs=topic_probs)
    else:
        rows, n_rows = sc.score_topk_masked(q_ptr, q_terms, mask_id, k_fb, topic_probs=topic_probs)
    n_q = len(n_rows)
    t_hit, w_hit, cnt = bi.doc_top_terms(np.ascontiguousarray(rows["doc"]).reshape(-1), m_doc)
    t_hit, w_hit, cnt = t_hit.reshape(n_q, k_fb, m_doc), w_hit.reshape(n_q, k_fb, m_doc), cnt.reshape(n_q, k_fb)
    terms, score, n_out = np.zeros((n_q, m), np.uint32), np.zeros((n_q, m), np.float64), np.zeros(n_q, np.int32)
    qp = np.asarray(q_ptr).astype(np.int64)
    for q in range(n_q):
        typed = {int(t) for t in np.asarray(q_terms)[qp[q]:qp[q + 1]]}
        addends = {}
        for j in range(int(n_rows[q])):
            for i in range(int(cnt[q, j])):
                if int(t_hit[q, j, i]) not in typed:
                    addends.setdefault(int(t_hit[q, j, i]), []).append(w_hit[q, j, i])
        cand = list(addends)
        sums = [rtm.sum_in_order(addends[t]) for t in cand]
        pick = rtm.candidate_order(cand, sums)[:m]
        n_out[q] = len(pick)
        terms[q, :len(pick)] = [cand[i] for i in pick]
        score[q, :len(pick)] = [sums[i] for i in pick]
    return terms, score, n_out


# (k_fb, m_doc, m): the issue's four, then the two sides of the 1024-slot threshold between the kernel's two workgroup sizes
CASES = [(1, 1, 1), (10, 5, 10), (64, 5, 64), (3, 64, 7), (64, 16, 10), (64, 17, 10)]


@pytest.mark.parametrize("with_prior", [False, True], ids=["no-prior", "prior"])
@pytest.mark.parametrize("k_fb,m_doc,m", CASES)
def test_rows_equal_reference_and_composition(ss_ctx, oracle, world, scorer, k_fb, m_doc, m, with_prior):
    sc, ti, bi = scorer
    q_ptr, q_terms = world["q_ptr"], world["q_terms"]
    probs = world["probs"] if with_prior else None
    if with_prior:
        sc.set_prior(world["prior"])
    got = sc.related_terms(q_ptr, q_terms, m=m, k_fb=k_fb, m_doc=m_doc, topic_probs=probs)
    want, n_rows = reference(oracle, world, k_fb, m_doc, m, with_prior)
    same(got, want)
    same(got, composed(sc, bi, q_ptr, q_terms, k_fb, m_doc, m, topic_probs=probs))
    assert got[2][61] == 0 and n_rows[61] == 0                         # unknown terms only: no hits
    assert 0 < n_rows[63] < engine._lib.SS_MAX_FEEDBACK_DOCS           # the rare term: fewer hits than the largest k_fb
    for q in range(len(got[2])):                                       # no row offers a word the user typed
        assert not set(got[0][q, :got[2][q]].tolist()) & set(q_terms[q_ptr[q]:q_ptr[q + 1]].tolist())


def dense_world():
    """600 docs x 300 terms, 100 body terms per doc with weights in [1, 2); the query's two terms (0 and 1, each in half the docs)
    weigh 1e-3, so they are never among a doc's 64 heaviest: every one of the 64 x 64 slots is live."""
    rng = np.random.default_rng(43)
    n_docs, n_terms = 600, 300
    rows = []
    for d in range(n_docs):
        row = {int(t): float(w) for t, w in zip(rng.choice(np.arange(2, n_terms), size=100, replace=False), 1.0 + rng.random(100))}
        for t in (0, 1):
            if rng.random() < 0.5:
                row[t] = 1e-3
        rows.append(row)
    body = table_of(rows, n_terms)
    title = table_of([{299: 1.0} if d % 7 == 0 else {} for d in range(n_docs)], n_terms)
    mb = np.sqrt(np.array([sum(float(np.float32(w)) ** 2 for w in r.values()) for r in rows]))
    return n_docs, title, body, np.ones(n_docs), mb


@pytest.mark.parametrize("m", [64, 1])
def test_all_4096_slots_live(ss_ctx, oracle, m):
    n_docs, title, body, mt, mb = dense_world()
    q_ptr, q_terms = np.array([0, 2], np.uint32), np.array([0, 1], np.uint32)
    rows, n_rows = oracle.score_topk_batch(n_docs, title, body, mt, mb, q_ptr, q_terms, 64)
    view = dvm.doc_view(*body, n_docs)
    t_hit, _, cnt = dvm.top_terms(view, rows["doc"][0], 64)
    assert n_rows[0] == 64 and (np.diff(view[0].astype(np.int64))[rows["doc"][0].astype(np.int64)] >= 64).all()
    assert (cnt == 64).all() and not np.isin(t_hit, q_terms).any()                  # 4096 live slots
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        bi.build_doc_view()
        got = sc.related_terms(q_ptr, q_terms, m=m, k_fb=64, m_doc=64)
        same(got, rtm.related_ref(rows, n_rows, view, q_ptr, q_terms, 64, m))
        assert got[2][0] == m
    finally:
        close_all(sc, ti, bi)


F32 = np.float32
# five docs, ranked 0 .. 4 by the typed term 0; the other terms carry the hostile weights
HOSTILE_DOCS = [
    {0: 5.0, 1: F32(1e-12), 2: F32("nan"), 3: F32(-0.0), 5: 2.0, 6: 2.0},
    {0: 4.0, 1: F32(1e3), 2: 1.0, 4: F32(-0.0), 5: 2.0, 6: 2.0},
    {0: 3.0, 1: F32(-1e3), 4: F32(0.0), 5: 2.0, 6: 2.0},
    {0: 2.0, 5: 2.0, 6: 2.0, 7: F32("nan")},
    {0: 1.0, 8: -1.0},
]


def hostile_world():
    body = table_of(HOSTILE_DOCS, 9)
    title = table_of([{}, {}, {}, {}, {8: 1.0}], 9)
    return 5, title, body, np.ones(5), np.ones(5)


def test_hostile_weights(ss_ctx, oracle):
    """NaN, -0.0, +0.0, equal weights and the order-sensitive triple 1e-12, 1e3, -1e3 in the stored weights.  (A sum starts from 0.0,
    so the term whose only weight is -0.0 scores +0.0 — 0.0 + -0.0 — and no sum can be -0.0: the model and the bits below say so.)"""
    n_docs, title, body, mt, mb = hostile_world()
    q_ptr, q_terms = np.array([0, 1], np.uint32), np.array([0], np.uint32)
    rows, n_rows = oracle.score_topk_batch(n_docs, title, body, mt, mb, q_ptr, q_terms, 5)
    assert n_rows[0] == 5 and rows["doc"][0].tolist() == [0, 1, 2, 3, 4]
    view = dvm.doc_view(*body, n_docs)
    want = rtm.related_ref(rows, n_rows, view, q_ptr, q_terms, 64, 16)
    in_order = rtm.sum_in_order([F32(1e-12), F32(1e3), F32(-1e3)])
    assert in_order.tobytes() != rtm.sum_in_order([F32(1e3), F32(-1e3), F32(1e-12)]).tobytes()
    # 5 and 6 tie at 8.0, then the triple's sum, the two zero sums by term id, -1.0, the NaN sums by term id
    assert want[2].tolist() == [8] and want[0][0, :8].tolist() == [5, 6, 1, 3, 4, 8, 2, 7]
    assert want[1][0, 2].tobytes() == in_order.tobytes() and want[1][0, :2].tolist() == [8.0, 8.0]
    assert want[1][0, 3:5].tobytes() == np.zeros(2).tobytes() and np.isnan(want[1][0, 6:8]).all()
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        bi.build_doc_view()
        got = sc.related_terms(q_ptr, q_terms, m=16, k_fb=5, m_doc=64)
        same(got, want)
        same(got, composed(sc, bi, q_ptr, q_terms, 5, 64, 16))
        # cut inside the tie at 8.0 and inside the NaNs
        for m in (1, 7):
            same(sc.related_terms(q_ptr, q_terms, m=m, k_fb=5, m_doc=64), rtm.related_ref(rows, n_rows, view, q_ptr, q_terms, 64, m))
    finally:
        close_all(sc, ti, bi)


def test_empty_answers(ss_ctx, oracle):
    """On the hand-worked table of test_related_terms_cpu.py: term 6 is only in doc 5, whose heaviest term it is (m_doc = 1: the hit
    holds nothing but the query term); an unknown term has no hits.  Both rows stay as the caller left them."""
    body = table_of(HAND_DOCS, 8)
    title = table_of([{}] * 5 + [{7: 1.0}], 8)
    sc, ti, bi = make_scorer(ss_ctx, 6, title, body, np.ones(6), np.ones(6))
    try:
        bi.build_doc_view()
        q_ptr, q_terms = np.array([0, 1, 2, 3], np.uint32), np.array([6, UNKNOWN, 0], np.uint32)
        out = (np.full((3, 4), 0xABABABAB, np.uint32), np.full((3, 4), -7.5), np.full(3, -5, np.int32))
        terms, score, n_out = sc.related_terms(q_ptr, q_terms, m=4, k_fb=3, m_doc=1, out=out)
        assert n_out.tolist() == [0, 0, 1]
        assert (terms[:2] == 0xABABABAB).all() and (score[:2] == -7.5).all()
        # query 2 (term 0: docs 0, 4, 1 by weight) is answered beside them: doc 0 and doc 4 give the typed term, doc 1 gives term 1 (a
        # weight tie with term 3); behind its one entry the row is untouched too
        rows, n_rows = oracle.score_topk_batch(6, title, body, np.ones(6), np.ones(6), q_ptr, q_terms, 3)
        want = rtm.related_ref(rows, n_rows, dvm.doc_view(*body, 6), q_ptr, q_terms, 1, 4)
        assert want[2].tolist() == [0, 0, 1] and want[0][2, 0] == 1 and want[1][2, 0] == 3.0
        assert terms[2, 0] == 1 and score[2, 0] == 3.0 and (terms[2, 1:] == 0xABABABAB).all() and (score[2, 1:] == -7.5).all()
    finally:
        close_all(sc, ti, bi)


def test_masks(ss_ctx, oracle, world, scorer):
    from tests.test_gpu_doc_masks import masked_ref
    sc, ti, bi = scorer
    q_ptr, q_terms = world["q_ptr"], world["q_terms"]
    n_q, k_fb, m_doc, m = len(q_ptr) - 1, 10, 5, 10
    rng = np.random.default_rng(44)
    allowed = rng.random((2, N_DOCS)) < 0.5
    sc.set_doc_masks(engine.pack_doc_masks(allowed, N_DOCS))
    mask_id = np.array([0, 1, -1, 1] * (n_q // 4), dtype=np.int32)
    got = sc.related_terms(q_ptr, q_terms, m=m, k_fb=k_fb, m_doc=m_doc, mask_id=mask_id)
    rows, n_rows = masked_ref(oracle, N_DOCS, world["title"], world["body"], world["mt"], world["mb"], q_ptr, q_terms, mask_id, allowed, k_fb)
    same(got, rtm.related_ref(rows, n_rows, world["view"], q_ptr, q_terms, m_doc, m))
    same(got, composed(sc, bi, q_ptr, q_terms, k_fb, m_doc, m, mask_id=mask_id))
    unmasked = reference(oracle, world, k_fb, m_doc, m, False)[0]
    assert got[0].tobytes() != unmasked[0].tobytes()                   # the lists change the answer
    for q in np.nonzero(mask_id == -1)[0]:
        assert got[0][q].tobytes() == unmasked[0][q].tobytes() and got[1][q].tobytes() == unmasked[1][q].tobytes()


def test_device_outputs(ss_ctx, oracle, world, scorer):
    import torch
    sc, ti, bi = scorer
    q_ptr, q_terms = world["q_ptr"], world["q_terms"]
    n_q, k_fb, m_doc, m = len(q_ptr) - 1, 10, 5, 10
    terms = torch.zeros(n_q * m, dtype=torch.int32, device="cuda")
    score = torch.zeros(n_q * m, dtype=torch.float64, device="cuda")
    n_out = torch.zeros(n_q, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(4):                                       # more calls than the scorer has turns: blocks and pinned staging are reused
        sc.related_terms(q_ptr, q_terms, m=m, k_fb=k_fb, m_doc=m_doc, out=(terms, score, n_out))
    got = (terms.cpu().numpy().view(np.uint32).reshape(n_q, m), score.cpu().numpy().reshape(n_q, m), n_out.cpu().numpy())
    same(got, reference(oracle, world, k_fb, m_doc, m, False)[0])
    same(got, sc.related_terms(q_ptr, q_terms, m=m, k_fb=k_fb, m_doc=m_doc))
    # without the scores
    terms2 = torch.zeros(n_q * m, dtype=torch.int32, device="cuda")
    n_out2 = torch.zeros(n_q, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sc.related_terms(q_ptr, q_terms, m=m, k_fb=k_fb, m_doc=m_doc, out=(terms2, None, n_out2))
    assert terms2.cpu().numpy().tobytes() == terms.cpu().numpy().tobytes() and n_out2.cpu().numpy().tolist() == got[2].tolist()
    # afterwards plain score_topk on the same scorer still equals the oracle
    h2, n2 = sc.score_topk(q_ptr, q_terms, 20)
    r2, rn2 = oracle.score_topk_batch(N_DOCS, world["title"], world["body"], world["mt"], world["mb"], q_ptr, q_terms, 20)
    assert_same_hits(h2, n2, r2, rn2)


def test_turn_blocks_regrown_under_queued_calls(ss_ctx, oracle, world, scorer):
    """Seven device-only calls back to back, more than twice the scorer's three turns, nothing waited for in between.  The batches
    hold 3, 40, 7, 64, 1, 64 and 5 of the world's queries, so the calls of 64 meet their turn's pinned blocks (the plan's, the queries'
    own terms') and device buffers too small and replace them while the two calls before them are still queued.  Every output then
    equals the host-output call on the same queries, byte for byte, and a plain score_topk afterwards still equals the oracle."""
    import torch
    sc, ti, bi = scorer
    lib = ss_ctx.lib
    q_ptr, q_terms = world["q_ptr"], world["q_terms"]
    k_fb, m_doc, m = 10, 5, 10
    calls = []
    for n, first in zip((3, 40, 7, 64, 1, 64, 5), (0, 11, 50, 0, 33, 0, 20)):
        calls.append({"n": n, "qp": (q_ptr[first:first + n + 1] - q_ptr[first]).astype(np.uint32),
                      "qt": np.ascontiguousarray(q_terms[q_ptr[first]:q_ptr[first + n]]),
                      "terms": torch.zeros(n * m, dtype=torch.int32, device="cuda"),
                      "score": torch.zeros(n * m, dtype=torch.float64, device="cuda"),
                      "n_out": torch.zeros(n, dtype=torch.int32, device="cuda")})
    torch.cuda.synchronize()
    for c in calls:
        rc = lib.ss_related_terms(sc.h, c["n"], c["qp"].ctypes.data, c["qt"].ctypes.data, None, None, None, k_fb, m_doc, m,
                                  c["terms"].data_ptr(), c["score"].data_ptr(), c["n_out"].data_ptr())
        assert rc == 0
    ss_ctx.synchronize()
    for c in calls:
        n = c["n"]
        got = (c["terms"].cpu().numpy().view(np.uint32).reshape(n, m), c["score"].cpu().numpy().reshape(n, m), c["n_out"].cpu().numpy())
        same(got, sc.related_terms(c["qp"], c["qt"], m=m, k_fb=k_fb, m_doc=m_doc))
    assert sum(int(c["n_out"].sum()) for c in calls) > 0
    # afterwards plain score_topk on the same scorer still equals the oracle (its rows computed once for the two routings)
    if "rows20" not in world["refs"]:
        world["refs"]["rows20"] = oracle.score_topk_batch(N_DOCS, world["title"], world["body"], world["mt"], world["mb"], q_ptr, q_terms, 20)
    h2, n2 = sc.score_topk(q_ptr, q_terms, 20)
    assert_same_hits(h2, n2, *world["refs"]["rows20"])


def test_refusals_leave_outputs_untouched(ss_ctx, oracle, world):
    sc, ti, bi = make_scorer(ss_ctx, N_DOCS, world["title"], world["body"], world["mt"], world["mb"])
    q_ptr, q_terms = world["q_ptr"][:5], world["q_terms"][:int(world["q_ptr"][4])]
    n_q = 4

    def refused(code, sc, **kw):
        args = {"m": 8, "k_fb": 10, "m_doc": 5}
        args.update(kw)
        out = (np.full((n_q, 65), 0xABABABAB, np.uint32), np.full((n_q, 65), -7.5), np.full(n_q, -5, np.int32))
        with pytest.raises(SpaghettiError) as ei:
            sc.related_terms(q_ptr, q_terms, out=out, **args)
        assert ei.value.code == code, kw
        assert (out[0] == 0xABABABAB).all() and (out[1] == -7.5).all() and (out[2] == -5).all(), kw
    try:
        refused(ERR_STATE, sc)                                                  # no view yet
        ti.build_doc_view()                                                     # the TITLE table's view does not count
        refused(ERR_STATE, sc)
        bi.build_doc_view()
        assert (sc.related_terms(q_ptr, q_terms)[2] > 0).all()
        for kw in ({"k_fb": 0}, {"k_fb": 65}, {"m_doc": 0}, {"m_doc": 65}, {"m": 0}, {"m": 65}):
            refused(ERR_INVALID, sc, **kw)
        refused(ERR_INVALID, sc, mask_id=np.array([-1, 0, -1, -1], np.int32))   # the scorer has no masks
        refused(ERR_INVALID, sc, mask_id=np.array([-1, -2, -1, -1], np.int32))
        refused(ERR_STATE, sc, topic_probs=np.full((n_q, K_TOPICS), 1.0 / K_TOPICS))       # no prior
        bad_ptr = q_ptr.copy()
        bad_ptr[2] = bad_ptr[1] - 1
        out = (np.full((n_q, 8), 0xABABABAB, np.uint32), np.full((n_q, 8), -7.5), np.full(n_q, -5, np.int32))
        with pytest.raises(SpaghettiError) as ei:
            sc.related_terms(bad_ptr, q_terms, m=8, out=out)
        assert ei.value.code == ERR_INVALID and (out[0] == 0xABABABAB).all() and (out[2] == -5).all()
        # the view goes with the weights (tfidf_build) and with the postings (apply_delta): a scorer made afterwards has none
        sc.close()
        bi.tfidf_build(N_DOCS, False, False, False)
        sc = engine.Scorer(ss_ctx, ti, bi)
        refused(ERR_STATE, sc)
        bi.build_doc_view()
        assert (sc.related_terms(q_ptr, q_terms)[2] > 0).all()
        sc.close()
        bi.apply_delta(del_docs=np.array([7], np.uint32), add=(np.array([3], np.uint32), np.array([7], np.uint32), np.array([0.5], np.float32)))
        sc = engine.Scorer(ss_ctx, ti, bi)
        refused(ERR_STATE, sc)
    finally:
        close_all(sc, ti, bi)


def test_host_mirror_related_terms(host, corpus, ss_ctx):
    """DeviceIndex.RelatedTerms on the config-1 corpus of test_gpu_host.py returns the word hashes of the term ids the engine call
    gives on the same tables (dense ids in sorted key order, as the host assigns them); it throws while SetSimilarPages is off."""
    import json
    from tests.test_gpu_host import _weighted_tables, h, oracle_index
    forw, inv = _weighted_tables(host, corpus)
    di = host.DeviceIndex()
    di.load(forw, inv)
    with pytest.raises(RuntimeError, match=r"switched off \(SetSimilarPages\)"):
        di.RelatedTerms("w3 w40")
    di.SetSimilarPages(True)
    docs_sorted = sorted(set(forw[3].keys()) | {d for t in (inv[0], inv[1]) for term in t.keys() for d in json.loads(t.get(term))})
    terms_sorted = sorted(set(inv[0].keys()) | set(inv[1].keys()))
    didx = {k: i for i, k in enumerate(docs_sorted)}
    tidx = {t: i for i, t in enumerate(terms_sorted)}
    title, body = (oracle_index({term: json.loads(t.get(term)) for term in t.keys()}, docs_sorted, terms_sorted) for t in (inv[0], inv[1]))
    mt, mb = np.zeros(len(docs_sorted)), np.zeros(len(docs_sorted))
    for d in forw[4].keys():
        row = json.loads(forw[4].get(d))
        mt[didx[d]], mb[didx[d]] = row.get("title", 0.0), row.get("body", 0.0)
    sc, ti, bi = make_scorer(ss_ctx, len(docs_sorted), title, body, mt, mb)
    try:
        bi.build_doc_view()
        for query, kw in (("w3 w40", {}), ("w149", {"m": 3, "k_fb": 4, "m_doc": 2}), ("w7 w90 w7", {"m": 64, "k_fb": 64, "m_doc": 64})):
            toks = query.split()
            q_terms = np.array([tidx.get(h(t), UNKNOWN) for t in toks], dtype=np.uint32)
            terms, _, n_out = sc.related_terms(np.array([0, len(toks)], np.uint32), q_terms, **kw)
            got = di.RelatedTerms(query, **kw)
            assert got == [terms_sorted[int(t)] for t in terms[0, :n_out[0]]] and len(got) > 0, query
            assert not set(got) & {h(t) for t in toks}
        assert di.RelatedTerms("notaword") == []
    finally:
        close_all(sc, ti, bi)
    di.SetSimilarPages(False)
    with pytest.raises(RuntimeError, match=r"switched off \(SetSimilarPages\)"):
        di.RelatedTerms("w3 w40")
