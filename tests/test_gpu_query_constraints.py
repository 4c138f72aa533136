"""GPU parity: required and excluded query terms (ss_score_topk_constrained) vs the CPU oracle and vs ss_score_topk_masked.

A doc is allowed for query q iff it is in q's registered allow-list (every doc for -1), contains every required term and no excluded
term (contains = has a title or a body posting of it).  The row is q's unrestricted ranking restricted to the allowed docs, so the
reference is the oracle on the tables with every posting of a disallowed doc deleted (test_gpu_doc_masks.masked_ref), and the same
call through ss_score_topk_masked with the allowed set registered must give the same bytes.  Every comparison is bit-exact.
"""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine, synth
from tests.test_gpu_doc_masks import masked_ref, random_masks, restrict_table
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)
from tests.test_gpu_score import assert_same_hits, build_weighted, close_all, make_scorer, tiny_index

pytestmark = pytest.mark.gpu

UNKNOWN = 0xFFFFFFFF


@pytest.fixture(autouse=True, params=[0, 1], ids=["small-kernel-off", "small-kernel-on"])
def _small_query_routing(request, ss_ctx):
    """As in test_gpu_doc_masks.py: every test runs with k_score_small off and with every query that fits sent there."""
    ss_ctx.set_option("score.small", request.param)
    yield
    ss_ctx.set_option("score.small", None)


# ---- reference construction -------------------------------------------------------------------------------------------------

class Contains:
    """contains(t) -> bool [n_docs]: the docs with a title or body posting of term t (no doc for an id >= n_terms)."""

    def __init__(self, n_docs, title, body):
        self.n_docs, self.tabs, self.memo = n_docs, (title, body), {}
        self.n_terms = len(title[0]) - 1

    def __call__(self, t):
        t = int(t)
        if t not in self.memo:
            c = np.zeros(self.n_docs, dtype=bool)
            if t < self.n_terms:
                for ptr, doc, _ in self.tabs:
                    c[np.asarray(doc)[int(ptr[t]):int(ptr[t + 1])].astype(np.int64)] = True
            self.memo[t] = c
        return self.memo[t]


def pack_pairs(lists):
    """[[ids of query 0], ...] -> (ptr [n_q + 1] uint32, terms uint32)."""
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    terms = np.array([t for x in lists for t in x], dtype=np.uint32)
    return ptr, terms


def allowed_sets(contains, n_docs, req, exc, mask_id=None, masks=None):
    """-> (set id per query, -1 = unconstrained and unmasked; bool [n_sets][n_docs]) with one set per distinct allowed set."""
    n_q = len(req)
    ids, sets, seen = np.full(n_q, -1, np.int32), [], {}
    for q in range(n_q):
        m = -1 if mask_id is None else int(mask_id[q])
        if not req[q] and not exc[q] and m < 0:
            continue
        a = np.ones(n_docs, dtype=bool) if m < 0 else masks[m].copy()
        for t in req[q]:
            a &= contains(t)
        for t in exc[q]:
            a &= ~contains(t)
        key = a.tobytes()
        if key not in seen:
            seen[key] = len(sets)
            sets.append(a)
        ids[q] = seen[key]
    return ids, (np.array(sets) if sets else np.zeros((0, n_docs), dtype=bool))


def check_batch(sc, oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, req, exc, k, mask_id=None, masks=None, prior=None,
                topic_probs=None, query_len=None):
    """The constrained call equals the oracle on the restricted tables, and ss_score_topk_masked over the same sets registered.
    Leaves `masks` (or nothing) registered again."""
    contains = Contains(n_docs, title, body)
    rp, rt = pack_pairs(req)
    ep, et = pack_pairs(exc)
    hits, n_hits = sc.score_topk_constrained(q_ptr, q_terms, k, req=(rp, rt), exc=(ep, et), mask_id=mask_id, query_len=query_len,
                                             topic_probs=topic_probs)
    ids, sets = allowed_sets(contains, n_docs, req, exc, mask_id, masks)
    ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, ids, sets, k, prior=prior, topic_probs=topic_probs,
                            query_len=query_len)
    assert_same_hits(hits, n_hits, ref, ref_n)
    sc.set_doc_masks(engine.pack_doc_masks(sets, n_docs) if len(sets) else None)
    mh, mn = sc.score_topk_masked(q_ptr, q_terms, ids if len(sets) else None, k, query_len=query_len, topic_probs=topic_probs)
    assert hits.tobytes() == mh.tobytes() and n_hits.tolist() == mn.tolist()
    sc.set_doc_masks(engine.pack_doc_masks(masks, n_docs) if masks is not None else None)
    return hits, n_hits


def random_constraints(rng, q_ptr, q_terms, n_terms, max_term):
    """0-3 required and 0-3 excluded terms per query: query terms, other terms, duplicates, unknown ids, a term both ways."""
    req, exc = [], []
    pool = lambda: int(min(rng.geometric(0.05) - 1, max_term))               # noqa: E731
    for q in range(len(q_ptr) - 1):
        qt = [int(x) for x in q_terms[q_ptr[q]:q_ptr[q + 1]]]
        r, e = [], []
        for lst, n in ((r, int(rng.integers(0, 4))), (e, int(rng.integers(0, 4)))):
            for _ in range(n):
                c = rng.random()
                if c < 0.35 and qt:
                    lst.append(qt[int(rng.integers(len(qt)))])
                elif c < 0.85:
                    lst.append(pool())
                elif c < 0.92:
                    lst.append(UNKNOWN)
                else:
                    lst.append(n_terms + int(rng.integers(0, 5)))
        if r and rng.random() < 0.15:
            r.append(r[0])                                                    # duplicate
        if r and rng.random() < 0.08:
            e.append(r[-1])                                                   # both required and excluded
        req.append(r)
        exc.append(e)
    return req, exc


# ---- tests --------------------------------------------------------------------------------------------------------------------

def test_kat(ss_ctx, oracle):
    """Hand-derived rows on the tiny index of test_gpu_score.py::test_kat (unrestricted query 0 = docs [2, 1, 3, 0])."""
    title, body, mag_t, mag_b = tiny_index()
    sc, ti, bi = make_scorer(ss_ctx, 5, title, body, mag_t, mag_b)
    try:
        contains = Contains(5, title, body)
        q_ptr = np.array([0, 2, 4, 6, 8, 10, 12], dtype=np.uint32)
        q_terms = np.array([0, 1] * 6, dtype=np.uint32)
        full, _ = sc.score_topk(q_ptr[:2], q_terms[:2], 10)
        assert full["doc"][0, :4].tolist() == [2, 1, 3, 0]
        t0, t1 = contains(0), contains(1)
        req = [[0], [1], [], [UNKNOWN], [0], [0, 0, 1]]
        exc = [[], [0], [1], [], [0], [UNKNOWN, 7]]
        hits, n_hits = check_batch(sc, oracle, 5, title, body, mag_t, mag_b, q_ptr, q_terms, req, exc, 10)
        order = full["doc"][0, :4].tolist()
        want = [[d for d in order if t0[d]], [d for d in order if t1[d] and not t0[d]], [d for d in order if not t1[d]], [], [],
                [d for d in order if t0[d] and t1[d]]]
        for q in range(6):
            assert hits["doc"][q, :n_hits[q]].tolist() == want[q], q
    finally:
        close_all(sc, ti, bi)


@pytest.mark.parametrize("n_docs,n_terms,p_body,p_title,n_q", [
    (3000, 200, 40000, 4000, 96),
    (60000, 3000, 900000, 60000, 160),          # multi-slice queries, several blocks of words per set
])
def test_random_batches(ss_ctx, oracle, n_docs, n_terms, p_body, p_title, n_q):
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, p_body, p_title, seed=n_docs + 17)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        rng = np.random.default_rng(n_q + 5)
        lens = rng.integers(1, 6, size=n_q)
        q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        q_terms = np.minimum(rng.geometric(0.02, size=int(lens.sum())) - 1, n_terms + 5).astype(np.uint32)
        req, exc = random_constraints(rng, q_ptr, q_terms, n_terms, n_terms - 1)
        for k in ((1, 10, 100, 300) if n_docs <= 3000 else (10, 300)):
            check_batch(sc, oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, req, exc, k)
        # combined with registered allow-lists
        masks = random_masks(n_docs, seed=n_q)
        sc.set_doc_masks(engine.pack_doc_masks(masks, n_docs))
        mask_id = rng.integers(-1, len(masks), size=n_q).astype(np.int32)
        for k in (10, 300):
            check_batch(sc, oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, req, exc, k, mask_id=mask_id, masks=masks)
    finally:
        close_all(sc, ti, bi)


def test_prior_topic_probs_and_query_len(ss_ctx, oracle):
    n_docs, n_terms = 40000, 1500
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 500000, 40000, seed=133)
    rng = np.random.default_rng(135)
    n_q = 96
    lens = rng.integers(1, 5, size=n_q)
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    q_terms = (rng.geometric(0.03, size=int(lens.sum())) - 1).clip(0, n_terms - 1).astype(np.uint32)
    req, exc = random_constraints(rng, q_ptr, q_terms, n_terms, n_terms - 1)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        prior = rng.random((16, n_docs)) * 1e-3
        probs = rng.dirichlet(np.ones(16), size=n_q)
        sc.set_prior(prior)
        check_batch(sc, oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, req, exc, 40, prior=np.ascontiguousarray(prior.T),
                    topic_probs=probs)
        sc.set_prior(None)
        qlen = rng.integers(1, 9, size=n_q).astype(np.int32)
        check_batch(sc, oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, req, exc, 40, query_len=qlen)
    finally:
        close_all(sc, ti, bi)


def test_phrase_queries(ss_ctx, oracle):
    from tests.test_gpu_phrase import positional_table
    n_docs, n_terms = 3000, 40
    (bt, bpos) = positional_table(n_docs, n_terms, 30000, seed=15)
    (tt, tpos) = positional_table(n_docs, n_terms, 4000, seed=16, max_pos=8, anchor_frac=0.5)
    wb, mb, _ = oracle.tfidf(*bt, n_docs, n_docs)
    wt, mt, _ = oracle.tfidf(*tt, n_docs, n_docs)
    title, body = (tt[0], tt[1], wt), (bt[0], bt[1], wb)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        ti.set_positions(*tpos)
        bi.set_positions(*bpos)
        contains = Contains(n_docs, title, body)
        cases = [([0, 3], [1, 2], [5], []), ([], [0, 1], [], [2]), ([5], [2, 0], [5, 6], [7]), ([2, 2], [1, 1], [UNKNOWN], []),
                 ([4], [0, 99], [], [4]), ([7, 1], [0, 1, 2], [3], [3]), ([9], [], [], []), ([], [3], [12], [13, UNKNOWN])]
        q_ptr, q_terms = pack_pairs([c[0] for c in cases])
        p_ptr, p_terms = pack_pairs([c[1] for c in cases])
        rp, rt = pack_pairs([c[2] for c in cases])
        ep, et = pack_pairs([c[3] for c in cases])
        for k in (20, 200):
            hits, n_hits = sc.score_topk_constrained(q_ptr, q_terms, k, req=(rp, rt), exc=(ep, et), p_ptr=p_ptr, p_terms=p_terms)
            sets = []
            for qi, (q, ph, r, e) in enumerate(cases):
                a = np.ones(n_docs, dtype=bool)
                for t in r:
                    a &= contains(t)
                for t in e:
                    a &= ~contains(t)
                sets.append(a)
                (t_, tp_), (b_, bp_) = restrict_table(title, a, tpos), restrict_table(body, a, bpos)
                extra = None
                if ph:
                    if all(x < n_terms for x in ph):
                        extra = oracle.phrase(t_, b_, tp_, bp_, ph)
                    else:
                        extra = (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
                ref, _ = oracle.score_topk(n_docs, t_, b_, mt, mb, np.array(q, np.uint32), k, query_len=len(q) + len(ph), extra=extra)
                n = int(n_hits[qi])
                assert n == len(ref), (qi, n, len(ref))
                assert hits[qi, :n]["doc"].tolist() == ref["doc"].tolist(), qi
                for f in ("title", "body", "final"):
                    assert np.array_equal(hits[f][qi, :n], ref[f]), (qi, f)
            sc.set_doc_masks(engine.pack_doc_masks(np.array(sets), n_docs))
            mh, mn = sc.score_topk_masked(q_ptr, q_terms, np.arange(len(cases), dtype=np.int32), k, p_ptr=p_ptr, p_terms=p_terms)
            assert hits.tobytes() == mh.tobytes() and n_hits.tolist() == mn.tolist()
            sc.set_doc_masks(None)
    finally:
        close_all(sc, ti, bi)


def _body_tables(lists, w):
    """Body postings = the lists (+ one term without body postings); title = one posting of that last term only."""
    b_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists]), [sum(len(x) for x in lists)]]).astype(np.uint64)
    body = (b_ptr, np.concatenate(lists).astype(np.uint32), np.asarray(w, np.float32))
    title = (np.array([0] * (len(lists) + 1) + [1], np.uint64), np.array([0], np.uint32), np.array([0.5], np.float32))
    return title, body


def test_adversarial_floor(ss_ctx, oracle):
    """Head terms as in test_gpu_doc_masks.py::test_adversarial_floor.  (a) A required term whose docs are every doc EXCEPT the
    top 256 postings of the query's head list: a floor from that list's k'-th largest impact would cut off every allowed doc.
    (b) An excluded term that holds exactly the query's unrestricted top k."""
    n_docs, n_heads, df = 40000, 6, 6000
    rng = np.random.default_rng(191)
    lists = [np.sort(rng.choice(n_docs, size=df, replace=False)) for _ in range(n_heads)]
    b_w_heads = [rng.uniform(0.05, 1.0, size=df).astype(np.float32) for _ in range(n_heads)]
    mb = rng.uniform(1.0, 2.0, size=n_docs)
    avoid = []
    for t in range(n_heads):
        imp = b_w_heads[t].astype(np.float64) / mb[lists[t]]
        top = lists[t][np.argsort(-imp, kind="stable")[:256]]
        avoid.append(np.setdiff1d(np.arange(n_docs), top))                   # term n_heads + t: every doc but those
    all_lists = lists + avoid
    b_w = np.concatenate(b_w_heads + [np.zeros(len(x), np.float32) for x in avoid])    # weight 0 postings still count
    title, body = _body_tables(all_lists, b_w)
    mt = np.ones(n_docs)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        q_ptr = np.arange(n_heads + 1, dtype=np.uint32)
        q_terms = np.arange(n_heads, dtype=np.uint32)
        for k in (10, 100):
            req = [[n_heads + t] for t in range(n_heads)]
            hits, n_hits = check_batch(sc, oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, req, [[]] * n_heads, k)
            assert (n_hits == k).all()
        # (b): the unrestricted top k of each query as the postings of an extra term
        k = 50
        full, _ = sc.score_topk(q_ptr, q_terms, k)
        extra = [np.sort(full["doc"][q, :k].astype(np.int64)) for q in range(n_heads)]
        t2, b2 = _body_tables(all_lists + extra, np.concatenate([b_w] + [np.ones(len(x), np.float32) for x in extra]))
    finally:
        close_all(sc, ti, bi)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, t2, b2, mt, mb)
    try:
        exc = [[2 * n_heads + q] for q in range(n_heads)]
        hits, n_hits = check_batch(sc, oracle, n_docs, t2, b2, mt, mb, q_ptr, q_terms, [[]] * n_heads, exc, k)
        assert (n_hits == k).all()
        for q in range(n_heads):
            assert not set(hits["doc"][q].tolist()) & set(extra[q].tolist())
    finally:
        close_all(sc, ti, bi)


def test_unconstrained_queries_keep_their_rows(ss_ctx, oracle):
    """Head-query batches that the routing sends to k_score_wave ("score.wave_min_list" = 0 at test sizes): the unconstrained
    queries of a constrained call equal ss_score_topk's rows; a call whose constraint arrays are NULL or all empty equals
    ss_score_topk_masked (and ss_score_topk)."""
    n_docs, n_terms = 300000, 20000
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 6000000, 400000, seed=144)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        q_ptr, q_terms = synth.make_queries(192, 3, 300, seed=146)
        rng = np.random.default_rng(18)
        for share in (0.1, 0.5):
            con = rng.random(192) < share
            req = [[int(rng.choice([3, 40, 250]))] if c and rng.random() < 0.5 else [] for c in con]
            exc = [[int(rng.choice([0, 7, 120]))] if c and not r else [] for c, r in zip(con, req)]
            for k in (50, 100):
                with ss_ctx.options(score__wave_min_list=0):
                    plain, pn = sc.score_topk(q_ptr, q_terms, k)
                    hits, n_hits = check_batch(sc, oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, req, exc, k)
                un = ~con
                assert hits[un].tobytes() == plain[un].tobytes() and n_hits[un].tolist() == pn[un].tolist()
        empty = (np.zeros(193, np.uint32), np.zeros(0, np.uint32))
        with ss_ctx.options(score__wave_min_list=0):
            plain, pn = sc.score_topk(q_ptr, q_terms, 100)
            masked, mn = sc.score_topk_masked(q_ptr, q_terms, None, 100)
            for req, exc in ((None, None), (empty, None), (None, empty), (empty, empty)):
                h, n = sc.score_topk_constrained(q_ptr, q_terms, 100, req=req, exc=exc)
                assert h.tobytes() == masked.tobytes() == plain.tobytes() and n.tolist() == mn.tolist() == pn.tolist()
            # only constraints that resolve to nothing (unknown excluded ids): the unconstrained rows
            h, n = sc.score_topk_constrained(q_ptr, q_terms, 100, exc=(np.arange(193, dtype=np.uint32), np.full(192, UNKNOWN, np.uint32)))
            assert h.tobytes() == plain.tobytes() and n.tolist() == pn.tolist()
    finally:
        close_all(sc, ti, bi)


def test_pipelined_constrained_batches(ss_ctx, oracle):
    """Device outputs on a stream shared with the caller: constrained batches with different sets back to back, unconstrained
    device-output calls and submit / collect tickets between them.  The caller's input arrays are scribbled on after every call
    and the outputs copied right behind it: every row must still be right (the set buffer lives as long as its batch)."""
    import torch
    n_docs, n_terms = 300000, 20000
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 6000000, 400000, seed=151)
    contains = Contains(n_docs, title, body)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ss_ctx.set_stream(stream.cuda_stream)
    sc = ti = bi = None
    try:
        with torch.cuda.stream(stream):
            sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
            rng = np.random.default_rng(163)
            batches = [synth.make_queries(96 + 48 * (i % 3), 3, 300, seed=170 + i) for i in range(9)]
            cons = []
            for qp, qt in batches:
                nq = len(qp) - 1
                req = [[int(rng.choice([9, 60, 333]))] if rng.random() < 0.4 else [] for _ in range(nq)]
                exc = [[int(rng.choice([1, 2])), int(rng.choice([500, 2000]))] if rng.random() < 0.4 else [] for _ in range(nq)]
                cons.append((req, exc))
            k = 40
            snaps, tickets = [], []
            with ss_ctx.options(score__wave_min_list=0):
                for i, ((qp, qt), (req, exc)) in enumerate(zip(batches, cons)):
                    nq = len(qp) - 1
                    qp, qt = qp.copy(), qt.copy()
                    (rp, rt), (ep, et) = pack_pairs(req), pack_pairs(exc)
                    out = (torch.zeros(nq * k * 40, dtype=torch.uint8, device=dev), torch.zeros(nq, dtype=torch.int32, device=dev))
                    if i % 3 == 2:
                        sc.score_topk(qp, qt, k, out=out)
                    else:
                        sc.score_topk_constrained(qp, qt, k, req=(rp, rt), exc=(ep, et), out=out)
                    snaps.append((out[0].clone(), out[1].clone()))
                    out[0].fill_(0xEE)
                    for a in (qt, rt, et):
                        a[:] = 0xFFFFFFFF
                    rp[1:] = 0
                    if i % 4 == 1:
                        tickets.append((i, sc.submit(*batches[i], k)))
                for i, tk in tickets:
                    h, n = sc.collect(tk)
                    ref, ref_n = oracle.score_topk_batch(n_docs, title, body, mt, mb, *batches[i], k)
                    assert_same_hits(h, n, ref, ref_n)
                stream.synchronize()
            for i, ((qp, qt), (req, exc), (dh, dn)) in enumerate(zip(batches, cons, snaps)):
                nq = len(qp) - 1
                if i % 3 == 2:
                    req, exc = [[]] * nq, [[]] * nq
                ids, sets = allowed_sets(contains, n_docs, req, exc)
                ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, qp, qt, ids, sets, k)
                hits = dh.cpu().numpy()[: nq * k * 40].view(engine.HIT_DTYPE).reshape(nq, k)
                assert_same_hits(hits, dn.cpu().numpy()[:nq], ref, ref_n)
    finally:
        for x in (sc, ti, bi):
            if x is not None:
                x.close()
        ss_ctx.set_stream(None)


def test_errors_leave_outputs_untouched(ss_ctx, oracle):
    import torch
    n_docs = 5000
    title, body, mt, mb = build_weighted(oracle, n_docs, 200, 50000, 5000, seed=13)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        sc.set_doc_masks(engine.pack_doc_masks(random_masks(n_docs, seed=14)[:3], n_docs))
        q_ptr, q_terms = synth.make_queries(4, 2, 50, seed=15)
        hits = np.zeros((4, 10), dtype=engine.HIT_DTYPE)
        hits["doc"] = 777
        n_hits = np.full(4, -5, np.int32)
        ok = (np.array([0, 1, 1, 2, 2], np.uint32), np.array([3, 4], np.uint32))
        many = (np.array([0, 17, 17, 17, 17], np.uint32), np.arange(17, dtype=np.uint32))
        cases = [  # (req, exc, mask_id, code)
            ((np.array([1, 1, 1, 2, 2], np.uint32), np.array([3, 4], np.uint32)), None, None, 1),      # does not start at 0
            ((np.array([0, 2, 1, 2, 2], np.uint32), np.array([3, 4], np.uint32)), None, None, 1),      # decreasing
            (None, (np.array([0, 1, 1, 2, 1], np.uint32), np.array([3, 4], np.uint32)), None, 1),
            (ok, None, np.array([0, 3, -1, 1], np.int32), 1),                                           # bad mask id
            (ok, None, np.array([-2, 0, 0, 0], np.int32), 1),
            (many, None, None, 7),                                                                       # 17 distinct terms
            ((np.array([0, 9, 9, 9, 9], np.uint32), np.arange(9, dtype=np.uint32)),
             (np.array([0, 8, 8, 8, 8], np.uint32), np.arange(100, 108, dtype=np.uint32)), None, 7),
        ]
        for req, exc, mid, code in cases:
            with pytest.raises(SpaghettiError) as ei:
                sc.score_topk_constrained(q_ptr, q_terms, 10, req=req, exc=exc, mask_id=mid)
            assert ei.value.code == code
            args = [None if x is None else x.ctypes.data for x in (req or (None, None)) + (exc or (None, None))]
            rc = ss_ctx.lib.ss_score_topk_constrained(sc.h, 4, q_ptr.ctypes.data, q_terms.ctypes.data, None, None, None, None,
                                                      None if mid is None else mid.ctypes.data, *args, 10, hits.ctypes.data,
                                                      n_hits.ctypes.data)
            assert rc == code
            assert (hits["doc"] == 777).all() and (n_hits == -5).all()
        # 16 distinct ids (duplicates do not count) are accepted
        sixteen = (np.array([0, 20, 20, 20, 20], np.uint32), np.concatenate([np.arange(16), np.arange(4)]).astype(np.uint32))
        sc.score_topk_constrained(q_ptr, q_terms, 10, req=sixteen)
        dev = torch.device("cuda", 0)
        dh = torch.full((4 * 10 * 40,), 0x5A, dtype=torch.uint8, device=dev)
        dn = torch.full((4,), -5, dtype=torch.int32, device=dev)
        for req, exc, mid, code in cases:
            with pytest.raises(SpaghettiError):
                sc.score_topk_constrained(q_ptr, q_terms, 10, req=req, exc=exc, mask_id=mid, out=(dh, dn))
        ss_ctx.synchronize()
        assert (dh.cpu() == 0x5A).all() and (dn.cpu() == -5).all()
    finally:
        close_all(sc, ti, bi)


def test_host_mirror_query_operators(host, corpus):
    """DeviceIndex.SetQueryOperators on the config-1 corpus of test_gpu_host.py: RetrieveBatch reads "+word" / "-word" and returns
    the unrestricted rows of the scored words (operators off, large k) restricted to the docs that contain every '+' word and no
    '-' word, cut at 50 — also through the masked overload.  With operators off, strings with '+' and '-' rank as they always did."""
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    word = corpus["word"]

    def contains(w):
        return {d for tab in (corpus["title"], corpus["body"]) for d in tab.get(h(w), {})}

    all_docs = set(corpus["doc"])
    # (query with operators, the same words as scored without them, required words, excluded words)
    cases = [("+w3 w17 -w40", "w3 w17", ["w3"], ["w40"]), ("w5 -w6 w7", "w5 w7", [], ["w6"]), ("+w1 +w2", "w1 w2", ["w1", "w2"], []),
             ('"w0 w1" +w3 -w2', '"w0 w1" w3', ["w3"], ["w2"]), ("-w3 w3", "w3", [], ["w3"]), ("w4 +nosuchword", "w4", ["nosuchword"], []),
             ("w2 w9 +w11-w12", "w2 w9 w11 w12", ["w11", "w12"], []), ("e-mail w60 - w70", "e-mail w60 - w70", [], []),
             ("w1 -nosuchword", "w1", [], [])]
    queries = [c[0] for c in cases]
    di = host.DeviceIndex()
    di.load(forw, inv)
    key = lambda rows: [(r.DocHash, r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in rows]      # noqa: E731
    off = di.RetrieveBatch(queries, 50)
    assert [key(r) for r in off] == [key(r) for r in di.RetrieveBatch([q.replace("+", " ").replace("-", " ") for q in queries], 50)]
    full = di.RetrieveBatch([c[1] for c in cases], 1024)
    di.SetQueryOperators(True)
    got = di.RetrieveBatch(queries, 50)
    n_nonempty = 0
    for (q, _, req, exc), g, f in zip(cases, got, full):
        allowed = set(all_docs)
        for w in req:
            allowed &= contains(w)
        for w in exc:
            allowed -= contains(w)
        want = [r for r in f if r.DocHash in allowed][:50]
        assert len(want) == 50 or len(f) < 1024, q
        assert key(g) == key(want), q
        n_nonempty += len(g) > 0
    assert n_nonempty >= 5
    # composed with an allow-list: a category's docs
    sets = host.TopicTeleportSets(forw, inv)
    cat = sorted(sets)[0]
    di.SetDocMasks({cat: sets[cat]})
    members = set(sets[cat])
    got = di.RetrieveBatch(queries, [cat, ""] * (len(queries) // 2) + [cat], 50)
    for i, ((q, _, req, exc), g, f) in enumerate(zip(cases, got, full)):
        allowed = set(all_docs) if i % 2 else set(members)
        for w in req:
            allowed &= contains(w)
        for w in exc:
            allowed -= contains(w)
        assert key(g) == key([r for r in f if r.DocHash in allowed][:50]), q
    di.SetQueryOperators(False)
    assert [key(r) for r in di.RetrieveBatch(queries, 50)] == [key(r) for r in off]
