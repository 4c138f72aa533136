"""GPU: the host mirror's late-interaction re-rank (DeviceIndex.SetDocTokens / RerankByMaxSim through pybind) on the golden 300 x 80
index with synthetic token vectors, against the engine's call on the same windows and token table and against the model
(tests/maxsim_model.py), by docHash.  The sort is stable in window order and never looks at the mirror's dense ids, so the pages are
compared exactly."""
import numpy as np
import pytest

from spaghettisearch_amd import engine
from tests import maxsim_model as mm
from tests.test_gpu_host import h, host  # noqa: F401  (module fixture of the host-mirror test)
from tests.test_gpu_host_facet import golden_tables
from tests.test_gpu_score import close_all
from tests.test_gpu_vector import tiny_scorer

pytestmark = pytest.mark.gpu

DIM = 64


def test_rerank_by_maxsim_equals_the_engine_call(host, ss_ctx):
    z, n_docs, n_terms, doc, forw, inv = golden_tables(host)
    di = host.DeviceIndex()
    di.load(forw, inv)
    rng = np.random.default_rng(47)
    queries = ["w3 w40 w79", "w12", "w0 w1 w2 w3 w4", "w9"]
    windows = [list(w) for w in di.RetrieveBatch(queries, 60)]
    assert max(len(w) for w in windows) > 10
    m_q = [3, 0, 17, 1]
    qtoks = [rng.integers(-8, 9, (m, DIM)).astype(np.int8) for m in m_q]
    with pytest.raises(RuntimeError, match="SetDocTokens"):
        di.RerankByMaxSim([q.tolist() for q in qtoks], windows)
    # 0 .. 5 token vectors for the first 250 pages (few distinct values: equal scores), none for the rest; a hash the index does not
    # hold is ignored
    named = 250
    counts = np.zeros(n_docs, np.int64)
    counts[:named] = rng.integers(0, 6, named)
    tok_ptr = np.zeros(n_docs + 1, np.uint64)
    tok_ptr[1:] = np.cumsum(counts)
    tok = np.zeros((int(tok_ptr[-1]), DIM), np.int8)
    tok[:, :4] = rng.integers(-8, 9, (len(tok), 4))
    tokens = {doc[d]: tok[int(tok_ptr[d]):int(tok_ptr[d + 1])].tolist() for d in range(named)}
    di.SetDocTokens({**tokens, h("http://nowhere/"): [[1] * DIM]})
    with pytest.raises(RuntimeError, match="length"):
        di.SetDocTokens({doc[0]: [[1] * 65]})
    with pytest.raises(RuntimeError, match="different lengths"):
        di.SetDocTokens({doc[0]: [[1] * 64, [1] * 128]})
    ghost = di.ScoreDocs("w0", [h("http://nowhere/")])[0]        # a row whose doc hash the index does not hold
    windows[0].insert(2, ghost)
    windows[3].append(ghost)
    at = {d: i for i, d in enumerate(doc)}
    k_in = max(len(w) for w in windows)
    hits = np.zeros((4, k_in), engine.HIT_DTYPE)
    n_hits = np.array([len(w) for w in windows], np.int32)
    for q, w in enumerate(windows):
        for j, r in enumerate(w):
            hits["doc"][q, j] = at.get(r.DocHash, n_docs)          # the golden numbering, the ghost outside
            hits["_pad"][q, j] = j
    qt_ptr = np.zeros(5, np.uint32)
    qt_ptr[1:] = np.cumsum(m_q)
    qtok = np.concatenate(qtoks)
    with pytest.raises(RuntimeError, match="one window per query"):
        di.RerankByMaxSim([q.tolist() for q in qtoks[:3]], windows)
    with pytest.raises(RuntimeError, match="wrong length"):
        di.RerankByMaxSim([[[1] * 65]] + [[]] * 3, windows)
    with pytest.raises(RuntimeError, match="ss_rerank_hits_by_maxsim"):
        di.RerankByMaxSim([[[1] * DIM] * 65] + [[]] * 3, windows)   # 65 query tokens
    sc, ti, bi = tiny_scorer(ss_ctx, n_docs)
    try:
        sc.set_doc_tokens(tok_ptr, tok)
        seen = 0
        for first, k in ((0, 60), (5, 10), (0, 1), (k_in - 2, 5), (k_in + 3, 2)):
            pages = di.RerankByMaxSim([q.tolist() for q in qtoks], windows, first, k)
            eng = sc.rerank_hits_by_maxsim(qt_ptr, qtok, hits, n_hits, k, first=first)
            want = mm.rerank(qt_ptr, qtok, tok_ptr, tok, hits, n_hits, first, k, np.zeros((4, k), engine.HIT_DTYPE), np.zeros(4, np.int32),
                             np.zeros((4, k), np.int32))
            assert eng[1].tolist() == want[1].tolist()
            for q, page in enumerate(pages):
                n = int(eng[1][q])
                assert eng[0]["_pad"][q, :n].tolist() == want[0]["_pad"][q, :n].tolist()
                rows = [windows[q][j] for j in eng[0]["_pad"][q, :n]]
                assert [r.DocHash for r in page.Results] == [r.DocHash for r in rows], (first, k, q)
                assert [r.FinalRank for r in page.Results] == [r.FinalRank for r in rows]
                assert list(page.Scores) == eng[2][q, :n].tolist() == want[2][q, :n].tolist()
                seen += n
        assert seen > 100
    finally:
        close_all(sc, ti, bi)
    # the ghost row and the pages without tokens come last, without a score; a query without tokens scores 0 where a doc has a token
    page = di.RerankByMaxSim([q.tolist() for q in qtoks], windows, 0, k_in)
    at_ghost = [r.DocHash for r in page[0].Results].index(ghost.DocHash)
    n_scored = sum(s != mm.NO_SCORE for s in page[0].Scores)
    assert at_ghost >= n_scored and set(page[0].Scores[n_scored:]) == {mm.NO_SCORE} and len(page[0].Results) == len(windows[0])
    assert set(page[1].Scores) <= {0, mm.NO_SCORE}
    di.SetDocTokens({})
    with pytest.raises(RuntimeError, match="SetDocTokens"):
        di.RerankByMaxSim([q.tolist() for q in qtoks], windows)
