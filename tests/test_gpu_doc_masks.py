"""GPU parity: top-k restricted to per-query doc allow-lists (ss_scorer_set_doc_masks, ss_score_topk_masked) vs the CPU oracle.

A doc's FinalRank depends only on its own postings, its own magnitudes and its own prior row (get_metadata.go:31-69), so the
exact answer of a query under allow-list M is the oracle's answer on the SAME tables with every posting of a disallowed doc
deleted (magnitudes kept as they are; positions deleted with their postings).  Every comparison is bit-exact.
"""
import json

import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine, synth
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)
from tests.test_gpu_score import assert_same_hits, build_weighted, close_all, make_scorer, tiny_index

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=[0, 1], ids=["small-kernel-off", "small-kernel-on"])
def _small_query_routing(request, ss_ctx):
    """As in test_gpu_score.py: every test runs with k_score_small off and with every query that fits sent there."""
    ss_ctx.set_option("score.small", request.param)
    yield
    ss_ctx.set_option("score.small", None)


# ---- reference construction -------------------------------------------------------------------------------------------------

def restrict_table(table, allowed, pos=None):
    """(term_ptr, post_doc, post_w) without the postings of disallowed docs; pos = (pos_ptr, pos) likewise."""
    ptr, doc, w = (np.asarray(a) for a in table)
    ptr = ptr.astype(np.int64)
    keep = allowed[doc.astype(np.int64)]
    term = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    cnt = np.bincount(term[keep], minlength=len(ptr) - 1)
    out = (np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), doc[keep].astype(np.uint32), w[keep].astype(np.float32))
    if pos is None:
        return out
    pp, pv = np.asarray(pos[0]).astype(np.int64), np.asarray(pos[1])
    plen = np.diff(pp)[keep]
    return out, (np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64), pv[np.repeat(keep, np.diff(pp))].astype(np.float32))


def sub_batch(ptr, terms, idx):
    ptr = np.asarray(ptr).astype(np.int64)
    parts = [np.asarray(terms)[ptr[i]:ptr[i + 1]] for i in idx]
    out = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint32), out


def masked_ref(oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, mask_id, allowed, k, prior=None, topic_probs=None, query_len=None):
    """The oracle per allow-list on that list's queries, over the posting-deleted tables.  allowed: bool [n_masks][n_docs]."""
    n_q = len(q_ptr) - 1
    mask_id = np.full(n_q, -1, np.int32) if mask_id is None else np.asarray(mask_id)
    hits = np.zeros((n_q, k), dtype=engine.HIT_DTYPE)
    n_hits = np.zeros(n_q, np.int32)
    for m in np.unique(mask_id):
        idx = np.nonzero(mask_id == m)[0]
        qp, qt = sub_batch(q_ptr, q_terms, idx)
        t, b = (title, body) if m < 0 else (restrict_table(title, allowed[m]), restrict_table(body, allowed[m]))
        kw = {}
        if prior is not None:
            kw = {"prior": prior, "topic_probs": topic_probs[idx]}
        if query_len is not None:
            kw["query_len"] = np.asarray(query_len)[idx]
        r, rn = oracle.score_topk_batch(n_docs, t, b, mt, mb, qp, qt, k, **kw)
        hits[idx], n_hits[idx] = r, rn
    return hits, n_hits


def random_masks(n_docs, seed):
    """Allow-lists of density 100 %, 50 %, 10 %, 1 %, a single doc and none."""
    rng = np.random.default_rng(seed)
    m = np.zeros((6, n_docs), dtype=bool)
    for i, dens in enumerate((1.0, 0.5, 0.1, 0.01)):
        m[i] = rng.random(n_docs) < dens
    m[4, int(rng.integers(n_docs))] = True
    return m


# ---- tests --------------------------------------------------------------------------------------------------------------------

def test_kat(ss_ctx, oracle):
    """Hand-derived rows on the tiny index of test_gpu_score.py::test_kat (unrestricted query 0 = docs [2, 1, 3, 0]) and on a table
    in which six docs tie exactly: an allow-list that cuts through the tie group keeps the survivors' ascending doc order."""
    title, body, mag_t, mag_b = tiny_index()
    sc, ti, bi = make_scorer(ss_ctx, 5, title, body, mag_t, mag_b)
    try:
        q_ptr = np.array([0, 2, 4, 6, 8], dtype=np.uint32)
        q_terms = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.uint32)
        allowed = np.array([[0, 1, 0, 1, 0], [1, 0, 1, 0, 0], [0, 0, 0, 0, 1], [1, 1, 1, 1, 1]], dtype=bool)
        sc.set_doc_masks(engine.pack_doc_masks(allowed, 5))
        full, fn = sc.score_topk(q_ptr[:2], q_terms[:2], 10)
        assert full["doc"][0, :4].tolist() == [2, 1, 3, 0]
        mask_id = np.array([0, 1, 2, 3], np.int32)
        hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 10)
        assert n_hits.tolist() == [2, 2, 0, 4]
        assert hits["doc"][0, :2].tolist() == [1, 3] and hits["doc"][1, :2].tolist() == [2, 0]
        for q, docs in ((0, [1, 3]), (1, [2, 0]), (3, [2, 1, 3, 0])):
            row = [int(np.nonzero(full["doc"][0, :4] == d)[0][0]) for d in docs]
            assert hits[q, :len(docs)].tobytes() == full[0, row].tobytes()        # the unrestricted rows themselves
        ref, ref_n = masked_ref(oracle, 5, title, body, mag_t, mag_b, q_ptr, q_terms, mask_id, allowed, 10)
        assert_same_hits(hits, n_hits, ref, ref_n)
        h1, n1 = sc.score_topk_masked(q_ptr, q_terms, mask_id, 1)
        assert n1.tolist() == [1, 1, 0, 1] and h1["doc"][:, 0].tolist() == [1, 2, 0, 2]
    finally:
        close_all(sc, ti, bi)
    # a tie group: docs 0..5 hold the same posting weight under the same magnitude, doc 6 more, doc 7 less
    n = 8
    b = (np.array([0, 8], np.uint64), np.arange(8, dtype=np.uint32), np.array([1, 1, 1, 1, 1, 1, 4, 0.5], np.float32))
    t = (np.array([0, 1], np.uint64), np.array([7], np.uint32), np.array([0.0], np.float32))
    mb, mt = np.ones(n), np.ones(n)
    sc, ti, bi = make_scorer(ss_ctx, n, t, b, mt, mb)
    try:
        allowed = np.zeros((2, n), dtype=bool)
        allowed[0, [1, 3, 5, 7]] = True
        allowed[1, [0, 2, 6]] = True
        sc.set_doc_masks(engine.pack_doc_masks(allowed, n))
        qp, qt = np.array([0, 1, 2, 3], np.uint32), np.array([0, 0, 0], np.uint32)
        hits, n_hits = sc.score_topk_masked(qp, qt, np.array([0, 1, -1], np.int32), 3)
        assert n_hits.tolist() == [3, 3, 3]
        assert hits["doc"].tolist() == [[1, 3, 5], [6, 0, 2], [6, 0, 1]]
        assert hits["final"][0, 0] == hits["final"][0, 2] == hits["final"][2, 1]
        ref, ref_n = masked_ref(oracle, n, t, b, mt, mb, qp, qt, [0, 1, -1], allowed, 3)
        assert_same_hits(hits, n_hits, ref, ref_n)
    finally:
        close_all(sc, ti, bi)


@pytest.mark.parametrize("n_docs,n_terms,p_body,p_title,n_q", [
    (3000, 200, 40000, 4000, 96),
    (60000, 3000, 900000, 60000, 160),          # multi-slice queries, compaction
])
def test_random_corpora(ss_ctx, oracle, n_docs, n_terms, p_body, p_title, n_q):
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, p_body, p_title, seed=n_docs + 7)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        allowed = random_masks(n_docs, seed=n_q)
        sc.set_doc_masks(engine.pack_doc_masks(allowed, n_docs))
        rng = np.random.default_rng(n_q + 1)
        lens = rng.integers(1, 6, size=n_q)
        q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        q_terms = np.minimum(rng.geometric(0.02, size=int(lens.sum())) - 1, n_terms + 5).astype(np.uint32)
        mask_id = rng.integers(-1, len(allowed), size=n_q).astype(np.int32)
        for k in (1, 10, 50, 100, 300, 1024):
            hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, k)
            ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, mask_id, allowed, k)
            assert_same_hits(hits, n_hits, ref, ref_n)
        if n_docs <= 3000:
            # cross-check: the unrestricted oracle ranking of every doc, masked and cut
            full, full_n = oracle.score_topk_batch(n_docs, title, body, mt, mb, q_ptr, q_terms, n_docs)
            hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 50)
            for q in range(n_q):
                row = full[q, :full_n[q]]
                if mask_id[q] >= 0:
                    row = row[allowed[mask_id[q]][row["doc"].astype(np.int64)]]
                row = row[:50]
                assert int(n_hits[q]) == len(row), q
                assert hits[q, :len(row)].tobytes() == row.tobytes(), q
    finally:
        close_all(sc, ti, bi)


def test_adversarial_floor(ss_ctx, oracle):
    """For every head term the allow-list excludes exactly the docs of that term's top 256 impacts: a threshold floor taken from
    the term's k'-th largest impact (k' = 16 for k = 10, 128 for k = 100) lies above every allowed doc's FinalRank and would cut
    them all off.  Body-only lists with distinct impacts (w / magnitude), so that no allowed doc ties with an excluded one and no
    title share lifts an allowed doc back over the floor.  Masked queries must not raise it."""
    n_docs, n_heads, df = 40000, 10, 6000
    rng = np.random.default_rng(91)
    lists = [np.sort(rng.choice(n_docs, size=df, replace=False)) for _ in range(n_heads)]
    b_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists]), [df * n_heads]]).astype(np.uint64)   # + one term without body postings
    b_doc = np.concatenate(lists).astype(np.uint32)
    b_w = rng.uniform(0.05, 1.0, size=len(b_doc)).astype(np.float32)
    body = (b_ptr, b_doc, b_w)
    title = (np.array([0] * (n_heads + 1) + [1], np.uint64), np.array([0], np.uint32), np.array([0.5], np.float32))   # (last term only)
    mb = rng.uniform(1.0, 2.0, size=n_docs)
    mt = np.ones(n_docs)
    allowed = np.ones((n_heads, n_docs), dtype=bool)
    for t in range(n_heads):
        lo, hi = int(b_ptr[t]), int(b_ptr[t + 1])
        imp = b_w[lo:hi].astype(np.float64) / mb[b_doc[lo:hi]]
        allowed[t, b_doc[lo:hi][np.argsort(-imp, kind="stable")[:256]]] = False
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        sc.set_doc_masks(engine.pack_doc_masks(allowed, n_docs))
        q_ptr = np.arange(n_heads + 1, dtype=np.uint32)
        q_terms = np.arange(n_heads, dtype=np.uint32)
        mask_id = np.arange(n_heads, dtype=np.int32)
        for k in (10, 100):
            hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, k)
            ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, mask_id, allowed, k)
            assert (ref_n == k).all()
            assert_same_hits(hits, n_hits, ref, ref_n)
    finally:
        close_all(sc, ti, bi)


def test_wave_batches(ss_ctx, oracle):
    """Head-query batches that the routing sends to k_score_wave (option "score.wave_min_list" = 0 at test sizes): the masked
    queries go to k_score_slices and are right; the unmasked queries of the same batch equal ss_score_topk's rows bit for bit."""
    n_docs, n_terms = 300000, 20000
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 6000000, 400000, seed=44)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        allowed = random_masks(n_docs, seed=5)[:4]
        sc.set_doc_masks(engine.pack_doc_masks(allowed, n_docs))
        q_ptr, q_terms = synth.make_queries(192, 3, 300, seed=46)
        rng = np.random.default_rng(8)
        for share in (0.1, 0.5):
            mask_id = np.where(rng.random(192) < share, rng.integers(0, 4, 192), -1).astype(np.int32)
            for k in (50, 100):
                with ss_ctx.options(score__wave_min_list=0):
                    plain, pn = sc.score_topk(q_ptr, q_terms, k)
                    hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, k)
                ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, mask_id, allowed, k)
                assert_same_hits(hits, n_hits, ref, ref_n)
                un = mask_id < 0
                assert hits[un].tobytes() == plain[un].tobytes() and n_hits[un].tolist() == pn[un].tolist()
    finally:
        close_all(sc, ti, bi)


def test_phrase_queries(ss_ctx, oracle):
    from tests.test_gpu_phrase import positional_table
    n_docs, n_terms = 3000, 40
    (bt, bpos) = positional_table(n_docs, n_terms, 30000, seed=5)
    (tt, tpos) = positional_table(n_docs, n_terms, 4000, seed=6, max_pos=8, anchor_frac=0.5)
    wb, mb, _ = oracle.tfidf(*bt, n_docs, n_docs)
    wt, mt, _ = oracle.tfidf(*tt, n_docs, n_docs)
    title, body = (tt[0], tt[1], wt), (bt[0], bt[1], wb)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        ti.set_positions(*tpos)
        bi.set_positions(*bpos)
        allowed = random_masks(n_docs, seed=12)[:4]
        sc.set_doc_masks(engine.pack_doc_masks(allowed, n_docs))
        cases = [([0, 3], [1, 2]), ([], [0, 1]), ([5], [2, 0]), ([2, 2], [1, 1]), ([4], [0, 99]), ([7, 1], [0, 1, 2]),
                 ([9], []), ([], [3]), ([1], [3, 2, 1, 0])]
        cases = cases * 4
        q_terms = np.array([t for q, _ in cases for t in q], dtype=np.uint32)
        q_ptr = np.concatenate([[0], np.cumsum([len(q) for q, _ in cases])]).astype(np.uint32)
        p_terms = np.array([t for _, ph in cases for t in ph], dtype=np.uint32)
        p_ptr = np.concatenate([[0], np.cumsum([len(ph) for _, ph in cases])]).astype(np.uint32)
        mask_id = np.repeat(np.array([-1, 0, 1, 2], np.int32), len(cases) // 4)
        tabs = {-1: (title, body, tpos, bpos)}
        for m in range(3):
            (rt, rtp), (rb, rbp) = restrict_table(title, allowed[m], tpos), restrict_table(body, allowed[m], bpos)
            tabs[m] = (rt, rb, rtp, rbp)
        for k in (20, 200):
            hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, k, p_ptr=p_ptr, p_terms=p_terms)
            for qi, (q, ph) in enumerate(cases):
                t, b, tp_, bp_ = tabs[int(mask_id[qi])]
                extra = None
                if ph:
                    if all(x < n_terms for x in ph):
                        extra = oracle.phrase(t, b, tp_, bp_, ph)
                    else:
                        extra = (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
                ref, _ = oracle.score_topk(n_docs, t, b, mt, mb, np.array(q, np.uint32), k, query_len=len(q) + len(ph), extra=extra)
                n = int(n_hits[qi])
                assert n == len(ref), (qi, n, len(ref))
                assert hits[qi, :n]["doc"].tolist() == ref["doc"].tolist(), qi
                for f in ("title", "body", "final"):
                    assert np.array_equal(hits[f][qi, :n], ref[f]), (qi, f)
        # no masked query: the phrase entry point's rows, bit for bit
        h0, n0 = sc.score_topk_phrase(q_ptr, q_terms, p_ptr, p_terms, 20)
        h1, n1 = sc.score_topk_masked(q_ptr, q_terms, None, 20, p_ptr=p_ptr, p_terms=p_terms)
        assert h0.tobytes() == h1.tobytes() and n0.tolist() == n1.tolist()
    finally:
        close_all(sc, ti, bi)


def test_prior_blend_exact_all_and_unclean_inputs(ss_ctx, oracle):
    n_docs, n_terms = 40000, 1500
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 500000, 40000, seed=33)
    allowed = random_masks(n_docs, seed=34)
    rng = np.random.default_rng(35)
    n_q = 96
    lens = rng.integers(1, 5, size=n_q)
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    q_terms = (rng.geometric(0.03, size=int(lens.sum())) - 1).clip(0, n_terms - 1).astype(np.uint32)
    mask_id = rng.integers(-1, len(allowed), size=n_q).astype(np.int32)
    packed = engine.pack_doc_masks(allowed, n_docs)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        sc.set_doc_masks(packed)
        # prior + topic_probs blend
        prior = rng.random((4, n_docs)) * 1e-3
        probs = rng.dirichlet(np.ones(4), size=n_q)
        sc.set_prior(prior)
        hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 40, topic_probs=probs)
        ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, mask_id, allowed, 40,
                                prior=np.ascontiguousarray(prior.T), topic_probs=probs)
        assert_same_hits(hits, n_hits, ref, ref_n)
        sc.set_prior(None)
        # every record through the exact stage, and a query length of its own
        qlen = rng.integers(1, 9, size=n_q).astype(np.int32)
        ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, q_ptr, q_terms, mask_id, allowed, 40, query_len=qlen)
        with ss_ctx.options(score__exact_all=1):
            hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 40, query_len=qlen)
        assert_same_hits(hits, n_hits, ref, ref_n)
        hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 40, query_len=qlen)
        assert_same_hits(hits, n_hits, ref, ref_n)
    finally:
        close_all(sc, ti, bi)
    # unclean inputs: negative weights and zero magnitudes (the filter is off for the call)
    (tp, td, tw), (bp, bd, bw) = title, body
    bw = bw.copy()
    bw[::7] *= -1.0
    mb2 = mb.copy()
    mb2[::11] = 0.0
    body2 = (bp, bd, bw)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body2, mt, mb2)
    try:
        sc.set_doc_masks(packed)
        hits, n_hits = sc.score_topk_masked(q_ptr, q_terms, mask_id, 40)
        ref, ref_n = masked_ref(oracle, n_docs, title, body2, mt, mb2, q_ptr, q_terms, mask_id, allowed, 40)
        assert_same_hits(hits, n_hits, ref, ref_n)
    finally:
        close_all(sc, ti, bi)


def test_no_regression_for_unmasked_calls(ss_ctx, oracle):
    n_docs, n_terms = 60000, 3000
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 900000, 60000, seed=21)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        q_ptr, q_terms = synth.make_queries(128, 3, 400, seed=22)
        before, bn = sc.score_topk(q_ptr, q_terms, 100)
        sc.set_doc_masks(engine.pack_doc_masks(random_masks(n_docs, seed=23), n_docs))
        after, an = sc.score_topk(q_ptr, q_terms, 100)
        assert before.tobytes() == after.tobytes() and bn.tolist() == an.tolist()
        for mid in (None, np.full(128, -1, np.int32)):
            h, n = sc.score_topk_masked(q_ptr, q_terms, mid, 100)
            assert h.tobytes() == before.tobytes() and n.tolist() == bn.tolist()
        sc.set_doc_masks(None)
        cleared, cn = sc.score_topk(q_ptr, q_terms, 100)
        assert cleared.tobytes() == before.tobytes()
        with pytest.raises(SpaghettiError):                                  # no masks any more: id 0 does not exist
            sc.score_topk_masked(q_ptr, q_terms, np.zeros(128, np.int32), 100)
    finally:
        close_all(sc, ti, bi)


def test_pipelined_masked_batches(ss_ctx, oracle):
    """Device outputs on a stream shared with the caller: masked batches back to back with different masks only enqueue; a
    copy of the outputs is enqueued right behind every call and checked.  set_doc_masks replaces the set between enqueued
    batches: the batches before it used the old set, those behind it the new one."""
    import torch
    n_docs, n_terms = 300000, 20000
    title, body, mt, mb = build_weighted(oracle, n_docs, n_terms, 6000000, 400000, seed=51)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ss_ctx.set_stream(stream.cuda_stream)
    sc = ti = bi = None
    try:
        with torch.cuda.stream(stream):
            sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
            set_a = random_masks(n_docs, seed=61)[:4]
            set_b = random_masks(n_docs, seed=62)[:4][::-1].copy()
            sc.set_doc_masks(engine.pack_doc_masks(set_a, n_docs))
            rng = np.random.default_rng(63)
            batches = [synth.make_queries(96 + 48 * (i % 3), 3, 300, seed=70 + i) for i in range(8)]
            mids = [rng.integers(-1, 4, size=len(qp) - 1).astype(np.int32) for qp, _ in batches]
            k = 40
            snaps, sets = [], []
            with ss_ctx.options(score__wave_min_list=0):
                for i, ((qp, qt), mid) in enumerate(zip(batches, mids)):
                    if i == 4:
                        sc.set_doc_masks(engine.pack_doc_masks(set_b, n_docs))
                    nq = len(qp) - 1
                    out = (torch.zeros(nq * k * 40, dtype=torch.uint8, device=dev), torch.zeros(nq, dtype=torch.int32, device=dev))
                    sc.score_topk_masked(qp, qt, mid, k, out=out)
                    snaps.append((out[0].clone(), out[1].clone()))
                    out[0].fill_(0xEE)
                    sets.append(set_a if i < 4 else set_b)
                stream.synchronize()
            for (qp, qt), mid, allowed, (dh, dn) in zip(batches, mids, sets, snaps):
                nq = len(qp) - 1
                ref, ref_n = masked_ref(oracle, n_docs, title, body, mt, mb, qp, qt, mid, allowed, k)
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
    title, body, mt, mb = build_weighted(oracle, n_docs, 200, 50000, 5000, seed=3)
    sc, ti, bi = make_scorer(ss_ctx, n_docs, title, body, mt, mb)
    try:
        sc.set_doc_masks(engine.pack_doc_masks(random_masks(n_docs, seed=4)[:3], n_docs))
        q_ptr, q_terms = synth.make_queries(4, 2, 50, seed=5)
        hits = np.zeros((4, 10), dtype=engine.HIT_DTYPE)
        hits["doc"] = 777
        n_hits = np.full(4, -5, np.int32)
        for bad in ([0, 3, -1, 1], [-2, 0, 0, 0], [0, 0, 0, 1 << 30]):
            with pytest.raises(SpaghettiError) as ei:
                sc.score_topk_masked(q_ptr, q_terms, np.array(bad, np.int32), 10)
            assert ei.value.code == 1
            rc = ss_ctx.lib.ss_score_topk_masked(sc.h, 4, q_ptr.ctypes.data, q_terms.ctypes.data, None, None, None, None,
                                                 np.array(bad, np.int32).ctypes.data, 10, hits.ctypes.data, n_hits.ctypes.data)
            assert rc == 1
            assert (hits["doc"] == 777).all() and (n_hits == -5).all()
        dev = torch.device("cuda", 0)
        dh = torch.full((4 * 10 * 40,), 0x5A, dtype=torch.uint8, device=dev)
        dn = torch.full((4,), -5, dtype=torch.int32, device=dev)
        with pytest.raises(SpaghettiError):
            sc.score_topk_masked(q_ptr, q_terms, np.array([0, 1, 2, 3], np.int32), 10, out=(dh, dn))
        ss_ctx.synchronize()
        assert (dh.cpu() == 0x5A).all() and (dn.cpu() == -5).all()
        assert ss_ctx.lib.ss_scorer_set_doc_masks(sc.h, -1, None) == 1
        assert ss_ctx.lib.ss_scorer_set_doc_masks(sc.h, 2, None) == 1
    finally:
        close_all(sc, ti, bi)


def test_host_mirror_search_within_category(host, corpus):
    """DeviceIndex.SetDocMasks + the masked RetrieveBatch on the config-1 corpus of test_gpu_host.py: "search within a category"
    with the doc sets of TopicTeleportSets equals the unrestricted RetrieveBatch at large k filtered by membership and cut at 50 —
    and still does after ApplyDelta re-created the scorer."""
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    rng = np.random.default_rng(8)
    cats = sorted(corpus["cats"])
    for wi in rng.choice(len(corpus["word"]), size=60, replace=False):         # ODP keyword vectors: word -> {category: frequency}
        cs = rng.choice(cats, size=int(rng.integers(1, 3)), replace=False)
        inv[2].set(h(corpus["word"][int(wi)]), json.dumps({str(c): int(rng.integers(1, 40)) for c in cs}))
    sets = host.TopicTeleportSets(forw, inv)
    assert sorted(sets) == cats and all(len(v) for v in sets.values())
    di = host.DeviceIndex()
    di.load(forw, inv)
    di.SetDocMasks({**sets, "hidden-nothing": [h("not a page")]})
    queries = ["w3 w17 w40", "w5 w6 w7", '"w3"', 'w40 "w0 w1"', "w1", "w2 w9 w11", "w60 w70"]

    def check():
        full = di.RetrieveBatch(queries, 1024)
        n_nonempty = 0
        for cat in cats:
            members = set(sets[cat])
            got = di.RetrieveBatch(queries, [cat] * len(queries), 50)
            for q, g, f in zip(queries, got, full):
                want = [r for r in f if r.DocHash in members][:50]
                assert len(want) == 50 or len(f) < 1024, q              # the unrestricted rows reach far enough to decide
                assert [(r.DocHash, r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in g] == \
                       [(r.DocHash, r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in want], (cat, q)
                n_nonempty += len(g) > 0
        assert n_nonempty >= len(cats)
        mixed = di.RetrieveBatch(queries, ["", cats[0], "hidden-nothing", cats[1], "", cats[2], cats[0]], 50)
        unres = di.RetrieveBatch(queries, 50)
        for i in (0, 4):
            assert [r.DocHash for r in mixed[i]] == [r.DocHash for r in unres[i]]
        assert mixed[2] == [] or all(r.DocHash == h("not a page") for r in mixed[2])
        with pytest.raises(Exception):
            di.RetrieveBatch(queries[:1], ["no such mask"], 50)

    check()
    doc, word = corpus["doc"], corpus["word"]
    page = doc[17]
    before = {"docHash": page,
              "title": {t: row[page] for t, row in corpus["title"].items() if page in row},
              "body": {t: row[page] for t, row in corpus["body"].items() if page in row},
              "children": corpus["children"][page], "anchors": {}}
    after = {"docHash": page, "title": {h(word[3]): [1.0, 0.0]},
             "body": {h(word[3]): [0.25, 4.0, 9.0], h(word[40]): [1.0, 0.0, 1.0, 2.0, 7.0]},
             "children": corpus["children"][page], "anchors": {}}
    di.ApplyDelta(forw, inv, before, after)
    check()
