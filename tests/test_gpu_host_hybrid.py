"""GPU: the host mirror's hybrid search (DeviceIndex.ScoreDocs / HybridSearch through pybind) on the config-1 corpus of
test_gpu_host.py, against the model's score (tests/hybrid_model.py: fuse_score) by docHash.  Dense ids are the mirror's own, so the two
windows come from the mirror's own RetrieveBatch and VectorSearch, and among rows of equal fused score any of them is right; the
engine's calls are compared byte for byte in test_gpu_hybrid.py."""
import numpy as np
import pytest

from tests import hybrid_model as hm
from tests import vector_model as vm
from tests.test_gpu_host import _weighted_tables, corpus, h, host  # noqa: F401  (module fixtures of the host-mirror test)

pytestmark = pytest.mark.gpu

DIM = 64


def test_score_docs_and_hybrid_search_follow_the_model(host, corpus):
    forw, inv = _weighted_tables(host, corpus)
    doc = corpus["doc"]
    di = host.DeviceIndex()
    di.load(forw, inv)
    rng = np.random.default_rng(43)
    queries = ["w3 w40 w149", "w120", "w7 w1 w2", "w0 w0", "neverseenword"]
    n_q = len(queries)
    qvec = rng.integers(-128, 128, (n_q, DIM)).astype(np.int8)
    with pytest.raises(RuntimeError, match="SetDocVectors"):
        di.HybridSearch(queries, qvec.tolist(), 10)
    named = 900
    vec = rng.integers(-128, 128, (named, DIM)).astype(np.int8)
    vectors = {doc[i]: vec[i].tolist() for i in range(named)}
    di.SetDocVectors(vectors)
    score = vm.scores(qvec, vec)
    at = {d: i for i, d in enumerate(doc[:named])}
    vec_score = lambda d, q: int(score[q, at[d]]) if d in at else 0          # noqa: E731

    # ---- ScoreDocs: the rows of a ranking are the rows of its docs; a doc the ranking does not reach has a row too
    unknown = h("http://nowhere/")
    for q, query in enumerate(queries[:4]):
        ranked = di.RetrieveBatch([query], 1000)[0]
        assert len(ranked) > 3
        hashes = [r.DocHash for r in ranked[::3]] + [unknown]
        rows = di.ScoreDocs(query, hashes)
        assert [r.DocHash for r in rows] == hashes
        for r, want in zip(rows, ranked[::3]):
            assert (r.TitleRank, r.BodyRank, r.PageRank, r.FinalRank) == (want.TitleRank, want.BodyRank, want.PageRank, want.FinalRank)
        assert (rows[-1].TitleRank, rows[-1].BodyRank, rows[-1].PageRank, rows[-1].FinalRank) == (0, 0, 0, 0)      # a hash the index does not hold
        outside = [d for d in doc if d not in {r.DocHash for r in ranked}][:5]
        for r in di.ScoreDocs(query, outside):
            assert (r.TitleRank, r.BodyRank, r.FinalRank) == (0, 0, 0)
    assert di.ScoreDocs("w3", []) == []
    assert len(di.ScoreDocs("w3", [doc[i % len(doc)] for i in range(1500)])) == 1500       # more than one window of SS_MAX_TOPK

    # ---- HybridSearch: the mirror's two windows fused by the model's score
    def check(k_window, params, fp, first, k, masks=None):
        lex = di.RetrieveBatch(queries, masks, k_window) if masks else di.RetrieveBatch(queries, k_window)
        near = di.VectorSearch(qvec.tolist(), k_window, masks or [])
        pages = di.HybridSearch(queries, qvec.tolist(), k_window, params, first, k, masks or [])
        assert len(pages) == n_q
        for q in range(n_q):
            lex_rank = {r.DocHash: i + 1 for i, r in enumerate(lex[q])}
            vec_rank = {r.DocHash: i + 1 for i, r in enumerate(near[q])}
            final = {r.DocHash: r.FinalRank for r in lex[q]}
            cands = sorted(set(lex_rank) | set(vec_rank))
            missing = [d for d in cands if d not in final]
            final.update({r.DocHash: r.FinalRank for r in di.ScoreDocs(queries[q], missing)})
            want = {d: float(hm.fuse_score(fp, lex_rank.get(d, 0), vec_rank.get(d, 0), final[d], vec_score(d, q))) for d in cands}
            page = pages[q]
            assert page.Union == len(cands)
            order = sorted(want.values(), reverse=True)[first:first + k]
            assert list(page.Scores) == order, (q, k_window, first, k)
            assert len({r.DocHash for r in page.Results}) == len(order)
            for r, s, vs, lr, vr in zip(page.Results, page.Scores, page.VecScores, page.LexRanks, page.VecRanks):
                d = r.DocHash
                assert want[d] == s and (lr, vr) == (lex_rank.get(d, 0), vec_rank.get(d, 0)) and vs == vec_score(d, q)
                assert r.FinalRank == final[d]
        return pages

    rrf, weighted = host.HybridParams(), host.HybridParams()
    weighted.weighted, weighted.w_vec = True, 1e-3
    pages = check(10, rrf, (hm.FUSE_RRF, 60, 1.0, 1.0), 0, 50)
    assert any(0 in p.LexRanks for p in pages) and any(0 in p.VecRanks for p in pages)
    assert pages[4].Union == 10 and set(pages[4].LexRanks) == {0}               # no known word: the vector window alone
    check(10, weighted, (hm.FUSE_WEIGHTED, 60, 1.0, 1e-3), 0, 50)
    check(60, rrf, (hm.FUSE_RRF, 60, 1.0, 1.0), 5, 7)
    check(1, weighted, (hm.FUSE_WEIGHTED, 60, 1.0, 1e-3), 0, 5)
    di.SetDocMasks({"some": [doc[i] for i in range(100, 200)]})
    pages = check(30, rrf, (hm.FUSE_RRF, 60, 1.0, 1.0), 0, 100, ["some", "", "some", "", "some"])
    assert {r.DocHash for r in pages[0].Results} <= {doc[i] for i in range(100, 200)}
    with pytest.raises(RuntimeError, match="quoted phrases"):
        di.HybridSearch(['w7 "w1 w2"'], qvec[:1].tolist(), 10)
    with pytest.raises(RuntimeError, match="one query vector per query"):
        di.HybridSearch(queries, qvec[:2].tolist(), 10)
