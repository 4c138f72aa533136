"""GPU parity: "similar pages" (ss_similar_topk) vs the numpy model + CPU oracle (tests/doc_view_model.similar_ref) and vs the same
answer composed from the public calls (ss_index_doc_top_terms -> ss_score_topk[_masked] at k + 1 -> drop the seed).  Every
comparison is bit-exact.
"""
import numpy as np
import pytest

from spaghettisearch_amd import SpaghettiError, engine
from tests import doc_view_model as dvm
from tests.test_gpu_host import corpus, host  # noqa: F401  (module fixtures of the host-mirror test)
from tests.test_gpu_score import assert_same_hits, build_weighted, close_all, make_scorer

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 7
N_DOCS, N_TERMS, K_TOPICS = 20000, 1000, 8


@pytest.fixture(autouse=True, params=[0, 1], ids=["small-kernel-off", "small-kernel-on"])
def _small_query_routing(request, ss_ctx):
    """As in test_gpu_query_constraints.py: every test runs with k_score_small off and with every query that fits sent there."""
    ss_ctx.set_option("score.small", request.param)
    yield
    ss_ctx.set_option("score.small", None)


@pytest.fixture(scope="module")
def world(oracle):
    """The tables, the seeds and the prior, built once: 64 random seeds, one seed without body postings, one doc listed twice."""
    title, body, mt, mb = build_weighted(oracle, N_DOCS, N_TERMS, 200000, 20000, 3)      # (seed 3: four docs have no body posting)
    rng = np.random.default_rng(32)
    lens = np.bincount(np.asarray(body[1]).astype(np.int64), minlength=N_DOCS)
    empty = np.nonzero(lens == 0)[0]
    assert len(empty), "the table has no doc without body postings"
    seeds = rng.choice(np.nonzero(lens > 0)[0], size=64, replace=False)
    seeds = np.concatenate([seeds, [empty[0]], [seeds[3]]]).astype(np.uint32)
    prior = rng.random((K_TOPICS, N_DOCS)) * 50.0
    probs = rng.dirichlet(np.ones(K_TOPICS), size=len(seeds))
    probs[65] = probs[3]                                  # the doc listed twice asks the same question twice
    return {"title": title, "body": body, "mt": mt, "mb": mb, "seeds": seeds, "prior": prior, "probs": probs, "refs": {}}


@pytest.fixture()
def scorer(ss_ctx, world):
    sc, ti, bi = make_scorer(ss_ctx, N_DOCS, world["title"], world["body"], world["mt"], world["mb"])
    bi.build_doc_view()
    yield sc, ti, bi
    close_all(sc, ti, bi)


def reference(oracle, world, k, m, with_prior):
    """similar_ref, computed once per (k, m, prior) and shared by the two routings"""
    key = (k, m, with_prior)
    if key not in world["refs"]:
        kw = {"prior": np.ascontiguousarray(world["prior"].T), "topic_probs": world["probs"]} if with_prior else {}
        world["refs"][key] = dvm.similar_ref(oracle, N_DOCS, world["title"], world["body"], world["mt"], world["mb"], world["seeds"], k, m, **kw)
    return world["refs"][key]


def composed(sc, bi, seeds, k, m, topic_probs=None, mask_id=None):
    """the definition through the public calls"""
    terms, _, cnt = bi.doc_top_terms(seeds, m, want_w=False)
    q_ptr, q_terms = dvm.queries_of(terms, cnt)
    if mask_id is None:
        rows, n_rows = sc.score_topk(q_ptr, q_terms, k + 1, topic_probs=topic_probs)
    else:
        rows, n_rows = sc.score_topk_masked(q_ptr, q_terms, mask_id, k + 1, topic_probs=topic_probs)
    return dvm.drop_seed(rows, n_rows, seeds, k)


@pytest.mark.parametrize("with_prior", [False, True], ids=["no-prior", "prior"])
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_rows_equal_reference_and_composition(ss_ctx, oracle, world, scorer, k, m, with_prior):
    sc, ti, bi = scorer
    seeds = world["seeds"]
    probs = world["probs"] if with_prior else None
    if with_prior:
        sc.set_prior(world["prior"])
    hits, n_hits = sc.similar_topk(seeds, k, m=m, topic_probs=probs)
    ref, ref_n = reference(oracle, world, k, m, with_prior)
    assert_same_hits(hits, n_hits, ref, ref_n)
    comp, comp_n = composed(sc, bi, seeds, k, m, topic_probs=probs)
    assert n_hits.tolist() == comp_n.tolist() and hits.tobytes() == comp.tobytes()          # byte for byte, zero rows included
    assert n_hits[64] == 0                                                                  # the seed without body postings
    assert hits[65].tobytes() == hits[3].tobytes() and n_hits[65] == n_hits[3]              # the doc listed twice
    for q in range(len(seeds)):
        assert int(seeds[q]) not in hits["doc"][q, :n_hits[q]].tolist()
    if with_prior:
        assert (hits["pagerank"][:64, 0] > 0).all()
    # afterwards plain score_topk on the same scorer still equals the oracle
    terms, _, cnt = dvm.top_terms(dvm.doc_view(*world["body"], N_DOCS), seeds[:16], 3)
    q_ptr, q_terms = dvm.queries_of(terms, cnt)
    h2, n2 = sc.score_topk(q_ptr, q_terms, 20)
    r2, rn2 = oracle.score_topk_batch(N_DOCS, world["title"], world["body"], world["mt"], world["mb"], q_ptr, q_terms, 20)
    assert_same_hits(h2, n2, r2, rn2)


def test_device_outputs(ss_ctx, oracle, world, scorer):
    import torch
    sc, ti, bi = scorer
    seeds, k, m = world["seeds"], 10, 5
    hits = torch.zeros(len(seeds) * k * engine.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    n_hits = torch.zeros(len(seeds), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(4):                                       # more calls than the scorer has turns: the turn's rows are reused
        sc.similar_topk(seeds, k, m=m, out=(hits, n_hits))
    got = hits.cpu().numpy().view(engine.HIT_DTYPE).reshape(len(seeds), k)
    ref, ref_n = reference(oracle, world, k, m, False)
    assert_same_hits(got, n_hits.cpu().numpy(), ref, ref_n)
    host_hits, host_n = sc.similar_topk(seeds, k, m=m)
    assert got.tobytes() == host_hits.tobytes()


def test_masks(ss_ctx, oracle, world, scorer):
    """One allow-list holds every seed, one excludes them all: under the excluding list nothing is dropped and the row is the first
    k rows of the masked ranking."""
    sc, ti, bi = scorer
    seeds, k, m = world["seeds"][:32], 10, 5
    rng = np.random.default_rng(33)
    allowed = rng.random((2, N_DOCS)) < 0.5
    allowed[0, seeds.astype(np.int64)] = True
    allowed[1, seeds.astype(np.int64)] = False
    sc.set_doc_masks(engine.pack_doc_masks(allowed, N_DOCS))
    mask_id = np.array([0, 1, -1, 1] * 8, dtype=np.int32)
    hits, n_hits = sc.similar_topk(seeds, k, m=m, mask_id=mask_id)
    ref, ref_n = dvm.similar_ref(oracle, N_DOCS, world["title"], world["body"], world["mt"], world["mb"], seeds, k, m, mask_id=mask_id,
                                 allowed=allowed)
    assert_same_hits(hits, n_hits, ref, ref_n)
    comp, comp_n = composed(sc, bi, seeds, k, m, mask_id=mask_id)
    assert n_hits.tolist() == comp_n.tolist() and hits.tobytes() == comp.tobytes()
    # the excluding list: the masked call at k itself
    terms, _, cnt = bi.doc_top_terms(seeds, m, want_w=False)
    q_ptr, q_terms = dvm.queries_of(terms, cnt)
    mh, mn = sc.score_topk_masked(q_ptr, q_terms, mask_id, k)
    for q in np.nonzero(mask_id == 1)[0]:
        assert hits[q].tobytes() == mh[q].tobytes() and n_hits[q] == mn[q]
    # a bad mask id: refused, outputs untouched
    out_h = np.frombuffer(bytearray(b"\x07" * (len(seeds) * k * engine.HIT_DTYPE.itemsize)), dtype=engine.HIT_DTYPE).reshape(len(seeds), k)
    out_n = np.full(len(seeds), -5, np.int32)
    bad = mask_id.copy()
    bad[5] = 2
    with pytest.raises(SpaghettiError) as ei:
        engine.check(sc.ctx.lib.ss_similar_topk(sc.h, len(seeds), seeds.ctypes.data, m, None, bad.ctypes.data, k, out_h.ctypes.data, out_n.ctypes.data), sc.ctx.h)
    assert ei.value.code == ERR_INVALID and (out_n == -5).all() and (out_h.view(np.uint8) == 7).all()


def test_limits_and_state(ss_ctx, world, scorer):
    sc, ti, bi = scorer
    seeds = world["seeds"][:4]
    for kwargs, code in (({"k": engine._lib.SS_MAX_TOPK}, ERR_UNSUPPORTED), ({"k": 0}, ERR_INVALID), ({"k": 5, "m": 0}, ERR_INVALID),
                         ({"k": 5, "m": 65}, ERR_INVALID)):
        with pytest.raises(SpaghettiError) as ei:
            sc.similar_topk(seeds, **kwargs)
        assert ei.value.code == code, kwargs
    with pytest.raises(SpaghettiError) as ei:
        sc.similar_topk(np.array([1, N_DOCS], np.uint32), 5)
    assert ei.value.code == ERR_INVALID
    h, n = sc.similar_topk(seeds, engine._lib.SS_MAX_TOPK - 1)                  # the largest k
    assert h.shape == (4, 1023) and (n > 0).all()
    bi.drop_doc_view()
    with pytest.raises(SpaghettiError) as ei:
        sc.similar_topk(seeds, 5)
    assert ei.value.code == ERR_STATE
    ti.build_doc_view()                                                         # the TITLE table's view does not count
    with pytest.raises(SpaghettiError) as ei:
        sc.similar_topk(seeds, 5)
    assert ei.value.code == ERR_STATE


def test_host_mirror_similar_pages(host, corpus):
    """DeviceIndex.SimilarPages on the config-1 corpus of test_gpu_host.py equals RetrieveBatch of the page's five heaviest body
    words at k + 1 without the page itself; switched off, the host builds no view."""
    import json
    from tests.test_gpu_host import _weighted_tables, h
    forw, inv = _weighted_tables(host, corpus)
    di = host.DeviceIndex()
    di.load(forw, inv)
    assert not di.HasDocView()                                                  # default off: nothing is built
    with pytest.raises(RuntimeError, match=r"switched off \(SetSimilarPages\)"):
        di.SimilarPages(corpus["doc"][3], 10)
    di.SetSimilarPages(True)
    assert di.HasDocView()
    word_of = {h(w): w for w in corpus["word"]}
    key = lambda res: [(r.DocHash, r.FinalRank, r.TitleRank, r.BodyRank, r.PageRank) for r in res]      # noqa: E731
    k = 20

    def body_rows():
        return {t: json.loads(inv[1].get(t)) for t in inv[1].keys()}

    def check(pages):
        for page in pages:
            top = di.DocTopTerms(page, 5)
            row = {t: np.float32(r[page][0]) for t, r in body_rows().items() if page in r}
            assert len(top) == min(5, len(row)) and len(set(top)) == len(top)
            weights = [row[t] for t in top]
            assert weights == sorted(row.values(), reverse=True)[:len(top)]      # the heaviest body words, heaviest first
            full = di.RetrieveBatch([" ".join(word_of[t] for t in top)], k + 1)[0]
            want = [r for r in full if r.DocHash != page][:k]
            got = di.SimilarPages(page, k)
            assert key(got) == key(want) and page not in [r.DocHash for r in got]
            assert len(got) == k
    check([corpus["doc"][i] for i in (3, 17, 500)])
    assert di.SimilarPages(h("not a page"), k) == []
    di.SetDocMasks({"some": corpus["doc"][:300]})
    got = di.SimilarPages(corpus["doc"][3], "some", k)
    assert got and all(r.DocHash in set(corpus["doc"][:300]) for r in got) and corpus["doc"][3] not in [r.DocHash for r in got]
    # after a delta re-created the scorer the view is there again, built from the updated table
    doc, word = corpus["doc"], corpus["word"]
    page = doc[17]
    before = {"docHash": page, "title": {t: r[page] for t, r in corpus["title"].items() if page in r},
              "body": {t: r[page] for t, r in corpus["body"].items() if page in r}, "children": corpus["children"][page], "anchors": {}}
    after = {"docHash": page, "title": {h(word[3]): [1.0, 0.0]}, "body": {h(word[3]): [0.25, 4.0, 9.0], h(word[40]): [1.0, 0.0, 1.0, 2.0, 7.0]},
             "children": corpus["children"][page], "anchors": {}}
    di.ApplyDelta(forw, inv, before, after)
    assert di.HasDocView()
    assert sorted(di.DocTopTerms(page, 5)) == sorted([h(word[3]), h(word[40])])
    check([corpus["doc"][3]])
    di.SetSimilarPages(False)
    assert not di.HasDocView()
